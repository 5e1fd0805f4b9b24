"""Drop-in for the reference's ``src/adapters`` operator package (hot-path subset): the same class
names, constructor arguments, ``forward(inputs, task, y=None)`` signature, config attribute names and
state-dict keys; the arithmetic runs in the fused HIP kernels.  Variants the kernels do not cover (other non-linearities, track_z,
low-rank adapters) run as plain torch ops (vl-pet_amd/eager.py: the eager fallback of SURVEY.md 8b).  Compacter's PHM adapters
(``HyperComplexAdapter``) generate their two weights with csrc/phm.hip and then run the same kernels; hyper-network adapters are a
baseline outside the VL-PET path and are not provided."""
from .config import AdapterConfig
from .adapter_modeling import Adapter, HyperComplexAdapter, LowRankAdapter, LowRankLinear
from .hypercomplex import PHMLinear
from .adapter_controller import AdapterController
from .adapter_utils import Activations

__all__ = ["AdapterConfig", "Adapter", "HyperComplexAdapter", "PHMLinear", "LowRankAdapter", "LowRankLinear", "AdapterController",
           "Activations"]
