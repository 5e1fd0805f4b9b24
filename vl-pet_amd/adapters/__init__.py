"""Drop-in for the reference's ``src/adapters`` operator package (hot-path subset): the same class
names, constructor arguments, ``forward(inputs, task, y=None)`` signature, config attribute names and
state-dict keys; the arithmetic runs in the fused HIP kernels.  Variants the kernels do not cover (other non-linearities, track_z,
low-rank adapters) run as plain torch ops (vl-pet_amd/eager.py: the eager fallback of SURVEY.md 8b).  Compacter's PHM adapters
(``HyperComplexAdapter``) generate their two weights with csrc/phm.hip and then run the same kernels; Hyperformer's hyper-networks (``adapter_hypernetwork``)
generate every layer's adapter weights with csrc/hyper.hip and hand them to the same kernels."""
from .config import AdapterConfig, MetaAdapterConfig
from .adapter_modeling import Adapter, HyperComplexAdapter, LowRankAdapter, LowRankLinear
from .hypercomplex import PHMLinear
from .adapter_controller import AdapterController
from .adapter_utils import Activations, TaskEmbeddingController, TaskHyperNet
from .adapter_hypernetwork import (AdapterLayersHyperNet, AdapterLayersHyperNetController, AdapterLayersOneHyperNetController,
                                   AdapterWeights, MetaLayersAdapterController)

__all__ = ["AdapterConfig", "Adapter", "HyperComplexAdapter", "PHMLinear", "LowRankAdapter", "LowRankLinear", "AdapterController",
           "Activations", "MetaAdapterConfig", "TaskEmbeddingController", "TaskHyperNet", "AdapterLayersHyperNet",
           "AdapterLayersHyperNetController", "AdapterLayersOneHyperNetController", "AdapterWeights", "MetaLayersAdapterController"]
