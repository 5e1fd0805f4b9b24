"""Bottleneck adapter (reference: adapters/adapter_modeling.py:36-61) and its low-rank and hypercomplex (Compacter) variants."""
import torch
import torch.nn as nn

from .adapter_utils import Activations
from .hypercomplex import PHMLinear, UNREACHABLE
from .. import functional as VF


class Adapter(nn.Module):
    """``up_sampler(act(down_sampler(x)))``.  Parameters are ordinary ``nn.Linear`` modules so the
    reference's checkpoints, init and name-substring freeze rules apply unchanged; the forward runs
    the fused HIP kernel (csrc/pet_fwd.hip)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.input_dim = config.d_model
        if config.use_adapter_down_dim:
            self.down_sample_size = config.adapter_down_dim
        else:
            self.down_sample_size = self.input_dim // config.reduction_factor
        self.activation = Activations(config.non_linearity.lower())
        # the fused kernels implement gelu_new and never materialise the [M, r] bottleneck: any other non-linearity, or track_z
        # (multitask.py:246-249 reads adapter.z), runs the plain-torch composition of vl-pet_amd/eager.py ("else eager
        # fallback"); no launch script of the reference asks for either
        self.eager = config.non_linearity.lower() != "gelu_new" or bool(config.track_z)
        self.down_sampler = nn.Linear(self.input_dim, self.down_sample_size)
        self.up_sampler = nn.Linear(self.down_sample_size, self.input_dim)
        self.track_z = config.track_z
        self._pack = VF.PackCache()

    def packed(self, io_dtype):
        return self._pack.get([self.down_sampler.weight], [self.down_sampler.bias], self.up_sampler.weight,
                              self.up_sampler.bias, io_dtype)

    def fused(self, x, residual, scale=1.0, link=None):
        """residual + scale * adapter(x) in one kernel (K2).  ``link``: functional.parallel_adapter."""
        if self.eager:
            out = self.forward(x)
            return residual + (out if scale == 1.0 else scale * out)
        pk = self.packed(VF._io_dtype(x))
        return VF.parallel_adapter(x, residual, self.down_sampler.weight, self.down_sampler.bias,
                                   self.up_sampler.weight, self.up_sampler.bias, pk, scale, link=link)

    def tail_weights(self):
        """(down weight [r, d], down bias, up weight [d, r], up bias) as ``adapter_tail.adapter_tail`` reads them (no autograd)"""
        return self.down_sampler.weight, self.down_sampler.bias, self.up_sampler.weight, self.up_sampler.bias

    def _keep_z(self, z):
        if self.track_z:
            self.z = z

    def forward(self, x):
        if self.eager:
            from .. import eager
            return eager.adapter(x, self.down_sampler.weight, self.down_sampler.bias, self.up_sampler.weight, self.up_sampler.bias,
                                 self.activation, self._keep_z)
        # bare adapter output (no residual): K1 kernel with gate off and x2_scale = 0
        pk = self.packed(VF._io_dtype(x))
        return VF.adapter_gate(None, x, [self.down_sampler.weight], [self.down_sampler.bias], self.up_sampler.weight,
                               self.up_sampler.bias, None, pk, None, VF.GATE_NONE, 1.0, 0.0, 1.0)


class LowRankLinear(nn.Module):
    """``x @ (W_left @ W_right) + b`` with rank-``rank`` factors (reference: adapters/low_rank_layer.py:8-46; parameter names kept)."""

    def __init__(self, input_dim: int, output_dim: int, rank: int = 1, bias: bool = True, w_init: str = "glorot-uniform"):
        super().__init__()
        self.input_dim, self.output_dim, self.rank, self.bias, self.w_init = input_dim, output_dim, rank, bias, w_init
        self.W_left = nn.Parameter(torch.empty(input_dim, rank))
        self.W_right = nn.Parameter(torch.empty(rank, output_dim))
        if bias:
            self.b = nn.Parameter(torch.zeros(output_dim))
        self.reset_parameters()

    def reset_parameters(self):
        if self.bias:
            nn.init.zeros_(self.b)
        if self.w_init == "glorot-uniform":
            nn.init.xavier_uniform_(self.W_left); nn.init.xavier_uniform_(self.W_right)
        elif self.w_init == "glorot-normal":
            nn.init.xavier_normal_(self.W_left); nn.init.xavier_normal_(self.W_right)
        else:
            raise ValueError(f"unknown low-rank init {self.w_init!r}")

    def forward(self, x):
        out = x @ (self.W_left @ self.W_right).to(x.dtype)
        return out + self.b.to(x.dtype) if self.bias else out


class LowRankAdapter(nn.Module):
    """Adapter whose two projections are low-rank products (reference: adapters/adapter_modeling.py:9-33).  One of the reference's
    baselines (outside the VL-PET hot path), so it runs as plain torch ops -- the eager fallback of SURVEY 8(b)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.input_dim = config.input_dim
        self.down_sample_size = self.input_dim // config.reduction_factor
        self.activation = Activations(config.non_linearity.lower())
        self.down_sampler = LowRankLinear(self.input_dim, self.down_sample_size, w_init=config.low_rank_w_init, rank=config.low_rank_rank)
        self.up_sampler = LowRankLinear(self.down_sample_size, self.input_dim, w_init=config.low_rank_w_init, rank=config.low_rank_rank)
        self.track_z = config.track_z
        self.eager = True

    def forward(self, x):
        z = self.activation(self.down_sampler(x))
        if self.track_z:
            self.z = z
        return self.up_sampler(z)

    def fused(self, x, residual, scale=1.0, link=None):
        out = self.forward(x)
        return residual + (out if scale == 1.0 else scale * out)


class HyperComplexAdapter(nn.Module):
    """Compacter's adapter (reference: adapters/adapter_modeling.py:88-139): a bottleneck adapter whose two projections are PHM layers.
    The parameters live in two ``PHMLinear`` modules (the reference's names and state-dict keys).  On the GPU the two nn.Linear-layout
    weights are generated by one launch (functional.phm_expand_pair, csrc/phm.hip) and handed, with the layers' own biases, to the
    kernels the plain ``Adapter`` runs: K2 (``fused``), K1 without a gate (``forward``), adapter_tail (decode).

    Staleness rule of the generated weights and their pack:
      * autograd on: the expansion and the pack run in EVERY forward (the pack into one buffer kept by this module).  A captured
        train step then contains both and reads the parameters in place; nothing here relies on ``functional.repack_all``, which
        does not know derived packs.
      * under ``no_grad``: weights and pack are cached on (data_ptr, _version) of the source parameters, ``functional.WEIGHTS_EPOCH``
        and the dtype, and on a miss are refreshed INTO THE SAME BUFFERS: a captured decode graph that has their addresses baked in
        keeps reading valid, current memory (the hazard ``functional.pack_pair(out=)`` documents).  Changes autograd's version
        counters do not see (``.data`` edits, raw-pointer writes) need ``functional.invalidate_caches()``, as everywhere.
    CPU tensors, a non-linearity other than gelu_new, ``track_z`` and a division outside 1 .. 8 run the plain-torch composition
    (vl-pet_amd/eager.py)."""

    def __init__(self, config):
        super().__init__()
        for name in UNREACHABLE:
            if getattr(config, name, False):
                raise ValueError(f"{name} is not supported (no launch flag of the reference reaches it)")
        self.config = config
        self.input_dim = config.input_dim
        if config.use_adapter_down_dim:
            self.down_sample_size = config.adapter_down_dim
        else:
            self.down_sample_size = self.input_dim // config.reduction_factor
        self.activation = Activations(config.non_linearity.lower())
        self.phm_dim = int(config.hypercomplex_division)
        kw = dict(bias=True, c_init=config.phm_c_init, phm_dim=self.phm_dim, learn_phm=config.learn_phm,
                  w_init=config.hypercomplex_nonlinearity, shared_phm_rule=config.shared_phm_rule, factorized_phm=config.factorized_phm,
                  phm_rank=config.phm_rank, phm_init_range=config.phm_init_range)
        self.down_sampler = PHMLinear(in_features=self.input_dim, out_features=self.down_sample_size, **kw)
        self.up_sampler = PHMLinear(in_features=self.down_sample_size, out_features=self.input_dim, **kw)
        self.track_z = config.track_z
        self.eager = (config.non_linearity.lower() != "gelu_new" or bool(config.track_z)
                      or not 1 <= self.phm_dim <= VF.PHM_MAX_DIVISION)
        self._wt = None         # (wt_d, wt_u) of the no_grad cache
        self._wt_key = None
        self._pack = VF.PackCache()     # no_grad: pack keyed on the source parameters
        self._train_pack = None         # autograd on: the one buffer every forward packs into

    def _sources(self):
        return self.down_sampler.sources() + self.up_sampler.sources() + [self.down_sampler.b, self.up_sampler.b]

    def _slices(self):
        return self.down_sampler.phm_rule, self.down_sampler.slices(), self.up_sampler.phm_rule, self.up_sampler.slices()

    def cached_weights(self):
        """(wt_d [r, d], wt_u [d, r]) without autograd, refreshed in place when a source parameter changed"""
        srcs = self._sources()
        key = (VF.WEIGHTS_EPOCH, srcs[1].dtype) + tuple((t.data_ptr(), t._version) for t in srcs)
        if key != self._wt_key:
            with torch.no_grad():
                self._wt = VF.phm_expand_pair_into(*self._slices(), self.phm_dim, out=self._wt)
            self._wt_key = key
        return self._wt

    def tail_weights(self):
        wt_d, wt_u = self.cached_weights()
        return wt_d, self.down_sampler.b, wt_u, self.up_sampler.b

    def _weights_and_pack(self, io_dtype):
        bd, bu = self.down_sampler.b, self.up_sampler.b
        if torch.is_grad_enabled():
            wt_d, wt_u = VF.phm_expand_pair(*self._slices(), self.phm_dim)
            self._train_pack = VF.pack_pair([wt_d], [bd], wt_u, bu, io_dtype, out=self._train_pack)
            return wt_d, wt_u, self._train_pack
        wt_d, wt_u = self.cached_weights()
        pk = self._pack.get_derived(self._sources(), ("phm", self.phm_dim), lambda: ([wt_d], [bd], wt_u, bu), io_dtype)
        return wt_d, wt_u, pk

    def _eager_path(self, x) -> bool:
        return self.eager or not x.is_cuda

    def fused(self, x, residual, scale=1.0, link=None):
        """residual + scale * adapter(x): the expansion, the pack and K2.  ``link``: functional.parallel_adapter."""
        if self._eager_path(x):
            out = self.forward(x)
            return residual + (out if scale == 1.0 else scale * out)
        wt_d, wt_u, pk = self._weights_and_pack(VF._io_dtype(x))
        return VF.parallel_adapter(x, residual, wt_d, self.down_sampler.b, wt_u, self.up_sampler.b, pk, scale, link=link)

    def _keep_z(self, z):
        if self.track_z:
            self.z = z

    def forward(self, x):
        if self._eager_path(x):
            from .. import eager
            d, u = self.down_sampler, self.up_sampler
            return eager.phm_adapter(x, d.phm_rule, d.slices(), d.b, u.phm_rule, u.slices(), u.b, self.activation, self._keep_z)
        wt_d, wt_u, pk = self._weights_and_pack(VF._io_dtype(x))
        return VF.adapter_gate(None, x, [wt_d], [self.down_sampler.b], wt_u, self.up_sampler.b, None, pk, None, VF.GATE_NONE,
                               1.0, 0.0, 1.0)
