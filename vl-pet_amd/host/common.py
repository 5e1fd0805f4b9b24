"""What the two host models (host/bart.py, host/t5.py) share, written once.  No A/B switches and no swappable hooks live here: the
harnesses set those as attributes of ``host.bart`` / ``host.t5``, and a helper that depends on one takes it as an argument."""
from __future__ import annotations

import contextlib
import copy

import torch

from .. import functional as VF
from ..adapters import AdapterConfig, AdapterController, MetaAdapterConfig
from ..prompt import EncoderPromptConfig


def derived_weights(owner, slot, mods, dtype):
    """``(cat of the modules' weights [sum out, in], cat of their biases or None)`` in ``dtype``: the fused q | k | v projection of a
    self-attention, the fused cross-attention key projection of a decoder.  A derived cache kept as the plain attribute ``slot`` of
    ``owner`` -- never a parameter or buffer: the state dict keeps the separate modules -- and rebuilt when one of the tensors
    changes (data pointer, version), after a cast of the frozen weights or a checkpoint load (functional.FROZEN_EPOCH).  The two halves
    are keyed apart, and a half with a TRAINABLE tensor in it (BitFit: the biases) also carries the optimizer's epoch
    (functional.WEIGHTS_EPOCH): the fused flat-buffer AdamW writes through raw pointers and bumps no version counter, so without it the
    fused bias would be as old as the cache."""
    def key_of(ts):
        k = tuple((t.data_ptr(), t._version) for t in ts) + (dtype, VF.FROZEN_EPOCH)
        return k + (VF.WEIGHTS_EPOCH,) if any(t.requires_grad for t in ts) else k
    ws = [m.weight for m in mods]
    bs = [] if mods[0].bias is None else [m.bias for m in mods]
    wkey, bkey = key_of(ws), key_of(bs)
    c = getattr(owner, slot, None)
    if c is None or c[0] != wkey or c[2] != bkey:
        with torch.no_grad():
            w = c[1] if (c is not None and c[0] == wkey) else torch.cat([t.to(dtype) for t in ws], 0).contiguous()
            b = None if not bs else (c[3] if (c is not None and c[2] == bkey) else torch.cat([VF.io_view(t, dtype) for t in bs], 0).contiguous())      # (io_view: a trainable bias comes from the trainer's IO shadow when that is current -- no cast launch)
        c = (wkey, w, bkey, b)
        setattr(owner, slot, c)
    return c[1], c[3]


def value_parallel_adapter(config) -> AdapterController:
    """K2 on the cross-attention value: the decoder's adapter config at its own down dim, parallel form, optional scaling"""
    ac = copy.deepcopy(config.adapter_config)
    ac.use_adapter_down_dim = True
    ac.adapter_down_dim = config.decoder_enc_attn_value_parallel_adapter_down_dim
    ac.use_parallel_adapter = True
    if config.use_decoder_enc_attn_value_parallel_adapter_scaling:
        ac.use_scaling_factor = True
        ac.scaling_factor = config.decoder_enc_attn_value_parallel_adapter_scaling_factor
    return AdapterController(ac)


GATE_FLAGS = ("use_encoder_adapter_gating_large_x_lowrank", "use_encoder_adapter_gating_small_xy_cat",
              "use_encoder_adapter_gating_middle_xy_add", "use_encoder_adapter_gating_middle_ia3_add")


def sequential_adapters(config, side: str) -> bool:
    """``side`` = "encoder" | "decoder": the Single-Adapter / Compacter placement -- an AdapterController behind every attention and
    feed-forward block of that stack (my_transformers/modeling_bart.py:932, 1525; modeling_t5.py:307, 350, 701, 744, 847)"""
    return bool(config.use_adapter or getattr(config, "use_compacter", False)) and not getattr(config, f"no_{side}_adapter")


# the Hyperformer flags of both hosts (param.py:147-157; scripts/image-text/hyperformer.sh: --use_hyperformer --unique_hyper_net
# --projected_task_embedding_dim 8 --reduction_factor 8); -1 = the config class's default (64)
HYPERFORMER_DEFAULTS = dict(use_hyperformer=False, unique_hyper_net=False, efficient_unique_hyper_net=False, projected_task_embedding_dim=-1)


def hyperformer(config) -> bool:
    return bool(getattr(config, "use_hyperformer", False))


def new_hyper_net(config, num_layers: int, include_cross_attention: bool):
    """the stack's controller as the reference picks it (my_transformers/modeling_bart.py:1980-1987, 2146-2153: the efficient form wins
    when both flags are set)"""
    from ..adapters import AdapterLayersHyperNetController, AdapterLayersOneHyperNetController
    ac = config.adapter_config
    cls = AdapterLayersOneHyperNetController if ac.efficient_unique_hyper_net else AdapterLayersHyperNetController
    return cls(ac, num_layers, include_cross_attention)


def block_adapters(hyper_net, task_embed, task, x):
    """every layer's generated adapters of one stack for ``task``: a list over layers of {block: AdapterWeights}, packed for the dtype of
    the activations ``x`` on the GPU -- ONE generator launch (none on a no_grad cache hit)"""
    io = VF._io_dtype(x) if x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) else None
    return hyper_net.generate(task_embed(task), task=task, io_dtype=io)


# the Compacter flags of both hosts (param.py:148-170, defaults as there; scripts/*/single_compacter.sh sets division 2, no shared rule,
# no factorization)
COMPACTER_DEFAULTS = dict(use_compacter=False, hypercomplex_division=4, phm_rank=1, shared_phm_rule=True, factorized_phm=True,
                          phm_init_range=0.01, shared_phm_rule_over_tasks=False)


# the prompt-tuning flags of both hosts (param.py:141-143 and --mid_dim; scripts/*/single_prompt.sh: 40, 800, single)
PROMPT_DEFAULTS = dict(encoder_prompt_len=0, decoder_prompt_len=0, mid_dim=768, use_single_prompt=False)


def make_prompt_config(c, task_list):
    """the ``encoder_prompt_config`` of a host config namespace (trainer_base.py:184-191), or None without ``encoder_prompt_len``;
    ``input_dim`` = the model's width (the reference leaves it at 768, the width of its backbones)"""
    if int(c.decoder_prompt_len) > 0:
        raise NotImplementedError("vl-pet_amd: decoder_prompt_len > 0 (the reference's decoder-prefix path, src/modeling_t5.py:642-645) "
                                  "is not provided: scripts/*/single_prompt.sh set encoder_prompt_len only")
    if int(c.encoder_prompt_len) < 0:
        raise ValueError("vl-pet_amd: encoder_prompt_len must not be negative")
    if int(c.encoder_prompt_len) == 0:
        return None
    return EncoderPromptConfig(prompt_len=int(c.encoder_prompt_len), seq_len=int(c.encoder_prompt_len), input_dim=c.d_model,
                               mid_dim=int(c.mid_dim), use_single_prompt=bool(c.use_single_prompt), tasks=list(task_list))


def make_adapter_config(c, task_list) -> AdapterConfig:
    """the ``adapter_config`` of a host config namespace (trainer_base.py:141-178); with ``use_compacter`` the hypercomplex fields"""
    if hyperformer(c):          # trainer_base.py:127-128, 143-146, 165-166: the MetaAdapterConfig with its class defaults
        ac = MetaAdapterConfig(tasks=task_list, input_dim=c.d_model, d_model=c.d_model, use_single_adapter=c.use_single_adapter,
                               reduction_factor=c.reduction_factor, use_adapter_down_dim=bool(c.use_adapter_down_dim),
                               adapter_down_dim=c.adapter_down_dim, unique_hyper_net=bool(c.unique_hyper_net),
                               efficient_unique_hyper_net=bool(c.efficient_unique_hyper_net))
        if int(c.projected_task_embedding_dim) != -1:
            ac.projected_task_embedding_dim = int(c.projected_task_embedding_dim)
        return ac
    ac = AdapterConfig(tasks=task_list, input_dim=c.d_model, d_model=c.d_model, use_single_adapter=c.use_single_adapter,
                       reduction_factor=c.reduction_factor, use_adapter_down_dim=bool(c.use_adapter_down_dim),
                       adapter_down_dim=c.adapter_down_dim)
    if c.use_compacter:
        ac.hypercomplex_adapters = True
        ac.hypercomplex_division, ac.phm_rank, ac.phm_init_range = c.hypercomplex_division, c.phm_rank, c.phm_init_range
        ac.shared_phm_rule, ac.factorized_phm = bool(c.shared_phm_rule), bool(c.factorized_phm)
        ac.shared_phm_rule_over_tasks = bool(c.shared_phm_rule_over_tasks)
    return ac


def install_shared_phm_rule(owner, roots, adapter_config) -> None:
    """``shared_phm_rule``: the model owns ONE rule and hands it to every PHMLinear under ``roots`` (src/modeling_bart.py:1480-1520,
    src/modeling_t5.py:454-499, with the init ranges used there).  As in the reference the parameter is registered under each layer
    as well, so the state dict lists it under all those names and ``named_parameters`` once, under the model's."""
    from ..adapters import PHMLinear
    ac = adapter_config
    if ac is None or not ac.hypercomplex_adapters or not ac.shared_phm_rule:
        return
    n = ac.hypercomplex_division
    owner.phm_rule = torch.nn.Parameter(torch.empty(n, n, n), requires_grad=bool(ac.learn_phm))
    with torch.no_grad():
        if ac.phm_c_init == "normal":
            owner.phm_rule.normal_(mean=0, std=ac.phm_init_range)
        elif ac.phm_c_init == "uniform":
            owner.phm_rule.uniform_(-1, 1)
        else:
            raise ValueError(f"phm_c_init {ac.phm_c_init!r}: normal or uniform")
    for root in roots:
        for m in root.modules():
            if isinstance(m, PHMLinear):
                m.set_phm_rule(owner.phm_rule)


def check_sequential_adapter_flags(config) -> None:
    """The launch scripts never combine sequential encoder adapters with the multi-head adapter (K1) or a gate, nor sequential decoder
    adapters with the value-parallel adapter; the reference resolves such a mix by the order of its if / elif chains.  Refused here
    rather than guessed.  More than one adapter kind at once is refused as there (trainer_base.py:125)."""
    kinds = [f for f in ("use_hyperformer", "use_adapter", "use_compacter") if getattr(config, f, False)]
    if len(kinds) > 1:
        raise ValueError(" and ".join(kinds) + ": at most one kind of adapters")
    if hyperformer(config):
        if not (config.unique_hyper_net or config.efficient_unique_hyper_net):
            raise ValueError("use_hyperformer needs unique_hyper_net or efficient_unique_hyper_net (my_transformers/modeling_bart.py:1987)")
        clash = [f for f in ("use_encoder_adapter_down_multihead", "use_decoder_enc_attn_value_parallel_adapter_down_dim", "use_lora")
                 + GATE_FLAGS if getattr(config, f, False)]
        if clash:
            raise ValueError("use_hyperformer (generated adapters behind every block of both stacks) cannot be combined with "
                             + ", ".join(clash))
    if sequential_adapters(config, "encoder"):
        clash = [f for f in ("use_encoder_adapter_down_multihead",) + GATE_FLAGS if getattr(config, f, False)]
        if clash:
            raise ValueError(f"{_kind(config)} with no_encoder_adapter=False (sequential encoder adapters) cannot be combined with "
                             + ", ".join(clash))
    if sequential_adapters(config, "decoder") and config.use_decoder_enc_attn_value_parallel_adapter_down_dim:
        raise ValueError(f"{_kind(config)} with no_decoder_adapter=False (sequential decoder adapters) cannot be combined with "
                         "use_decoder_enc_attn_value_parallel_adapter_down_dim")


def _kind(config) -> str:
    return "use_compacter" if getattr(config, "use_compacter", False) else "use_adapter"


def fused_adapter_tail(enabled, ctl, task, h, residual, norm, p, training):
    """The plain ``Adapter`` (or Compacter's ``HyperComplexAdapter``) of ``ctl`` for ``task`` when "adapter, then tail" may run as the
    one fused launch (vlpet_amd.adapter_tail), else None: switched on, on the GPU, no dropout, no gradient needed, a fused adapter
    with nothing around it inside the controller, a shape the kernel takes, at most ``ADAPTER_TAIL_MAX_ROWS`` rows.  The caller
    passes ``ad.tail_weights()`` to the kernel: the parameters themselves, or the cached expanded weights and ``b``."""
    from .. import adapter_tail as AT
    from ..adapters.adapter_modeling import Adapter, HyperComplexAdapter
    if not enabled or not h.is_cuda or (training and p > 0):
        return None
    cfg = ctl.config
    if cfg.use_parallel_adapter or ctl.add_layer_norm_before_adapter or ctl.add_layer_norm_after_adapter:
        return None
    ad = ctl.get_adapter(ctl.get_task(task))
    if type(ad) not in (Adapter, HyperComplexAdapter) or ad.eager:
        return None
    if torch.is_grad_enabled():
        params = list(ad.parameters()) + ([] if norm is None else list(norm.parameters()))
        if h.requires_grad or residual.requires_grad or any(t.requires_grad for t in params):
            return None
    d = h.shape[-1]
    M = h.numel() // d
    if M == 0 or M > AT.ADAPTER_TAIL_MAX_ROWS or not AT.applies(M, d, ad.down_sample_size, h.dtype):
        return None
    return ad


def fused_generated_tail(enabled, meta, w, h, residual, norm, p, training) -> bool:
    """``fused_adapter_tail`` for a GENERATED (wd, bd, wu, bu) set (Hyperformer): whether "adapter, then tail" may run as the one fused
    launch -- switched on, on the GPU, no dropout, no gradient needed, gelu_new without track_z, a shape the kernel takes."""
    from .. import adapter_tail as AT
    if not enabled or not h.is_cuda or (training and p > 0) or meta.eager or w.pack is None:
        return False
    if torch.is_grad_enabled():
        ts = [h, residual, *w.tail_weights()] + ([] if norm is None else list(norm.parameters()))
        if any(t.requires_grad for t in ts):
            return False
    d = h.shape[-1]
    M = h.numel() // d
    return 0 < M <= AT.ADAPTER_TAIL_MAX_ROWS and bool(AT.applies(M, d, w.down_w.shape[0], h.dtype))


def unpack_vis_inputs(vis_inputs, downsample, dtype):
    """(feats, boxes, img_ids or None, obj_ids or None) of the loader's visual tuple, the features in ``dtype``: through the
    encoder's ``Downsample`` when it has one (fp32 CLIP features -> compute dtype inside the pooling kernel; rounding is monotone:
    pool(round(f)) == round(pool(f))), else a cast"""
    if downsample is not None:
        vis_inputs = downsample(vis_inputs, out_dtype=dtype)
    elif vis_inputs[0].dtype != dtype:
        vis_inputs = (vis_inputs[0].to(dtype),) + tuple(vis_inputs[1:])
    return (vis_inputs[0], vis_inputs[1], vis_inputs[2] if len(vis_inputs) >= 3 else None,
            vis_inputs[3] if len(vis_inputs) == 4 else None)


def shift_right(labels, pad_id, start_id):
    """decoder inputs of ``labels``: BART's shift_tokens_right, T5PreTrainedModel._shift_right (my_transformers/modeling_t5.py:1068-1087)"""
    out = labels.new_zeros(labels.shape)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = start_id
    return out.masked_fill(out == -100, pad_id)


def is_key_mask(attn_mask) -> bool:
    """a boolean ``[B, 1, 1, L]`` mask: key padding only, the form the short-sequence attention kernels take as ``[B, L]``"""
    return attn_mask.dtype == torch.bool and attn_mask.dim() == 4 and attn_mask.shape[1] == 1 and attn_mask.shape[2] == 1


@contextlib.contextmanager
def eval_no_grad(model):
    """the frame of ``generate()``: eval mode without autograd; the mode the model was in is restored whatever happens inside"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)
