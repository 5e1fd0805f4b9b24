"""Minimal BART encoder-decoder host with the reference's PET hook points.

This is the frozen backbone the hot path plugs into: plain PyTorch-ROCm (library GEMMs, SDPA,
LayerNorm), no HIP code of ours -- the PET arithmetic is delegated to ``encoder_pet.apply_pet``
(K1), ``adapters.AdapterController`` (K2), ``lora.LoRALinearController`` (K3) and
``visual.VisualEmbedding`` (K4).  Module / parameter names follow the reference so that its
checkpoints and its name-substring freeze rules apply:

  model.shared, model.encoder.{embed_tokens,embed_positions,layernorm_embedding,visual_embedding},
  model.encoder.layers.{l}.{self_attn.{q,k,v,out}_proj,self_attn_layer_norm,fc1,fc2,final_layer_norm,
      attn_adapter_multihead_down.{h},attn_adapter_multihead_up,ff_adapter_multihead_*,
      encoder_{attn,ff}_adapter_gating_large_x_{down,up}},
  model.decoder.layers.{l}.{self_attn,encoder_attn.{...,attn_value_parallel_adapter.adapters.{task}},...}

Structure restated from: src/modeling_bart.py:696-900 (JointEncoder: text LN before concat
[text ; visual]), my_transformers/modeling_bart.py:1122-1380 (encoder layer, post-LN),
:1611-1760 (decoder layer), :397-566 (cross-attention with value-parallel adapter),
src/modeling_bart.py:1522-1602 (LM head + CE with reduction='none').
"""
from __future__ import annotations

import copy
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import attention as A
from .. import decode as D
from .. import functional as VF
from .. import adapter_tail as AT
from ..adapters import AdapterController, MetaLayersAdapterController, TaskEmbeddingController
from ..encoder_pet import apply_pet, build_pet, has_pet
from ..lora import LoRALinearController, LoraConfig
from ..visual import Downsample, LowRankVisualEmbedding, VisualEmbedding
from ..prompt import PromptController
from .common import (COMPACTER_DEFAULTS, HYPERFORMER_DEFAULTS, PROMPT_DEFAULTS, block_adapters, fused_generated_tail, hyperformer, new_hyper_net, check_sequential_adapter_flags, derived_weights, eval_no_grad, fused_adapter_tail,
                     install_shared_phm_rule, is_key_mask, make_adapter_config, make_prompt_config, sequential_adapters, shift_right, unpack_vis_inputs,
                     value_parallel_adapter)

TASKS = ["vqa", "gqa", "nlvr", "caption"]


def vlpet_config(**over) -> SimpleNamespace:
    """Config namespace with the attribute names the reference copies from its argparse flags onto the
    HF config (trainer_base.py:86-87).  Defaults = scripts/image-text/VL-PET-large.sh with r=96."""
    c = SimpleNamespace(
        # backbone (facebook/bart-base)
        d_model=768, encoder_layers=6, decoder_layers=6, encoder_attention_heads=12, decoder_attention_heads=12,
        encoder_ffn_dim=3072, decoder_ffn_dim=3072, vocab_size=50265 + 200, max_position_embeddings=1024,
        dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, pad_token_id=1, decoder_start_token_id=2,
        scale_embedding=False, init_std=0.02,
        # visual
        feat_dim=2048, pos_dim=4, n_images=2, n_boxes=36, downsample=True, use_vis_order_embedding=True,
        use_vis_layer_norm=True, individual_vis_layer_norm=True, share_vis_lang_layer_norm=False,
        use_lowrank_visual_projector=False, visual_projector_down_dim=96, visual_projector_multihead_num_head=1,
        use_visual_projector_gating_large_x_lowrank=False, visual_projector_gating_down_dim=96,
        use_visual_projector_residual_connection=False,
        # PET flags
        tasks=",".join(TASKS), use_adapter=True, use_single_adapter=True, no_encoder_adapter=True,
        no_decoder_adapter=True, add_adapter_cross_attn=True, use_adapter_down_dim=True, adapter_down_dim=96,
        use_encoder_adapter_down_multihead=True, encoder_adapter_multihead_num_head=4,
        use_encoder_adapter_gating_large_x_lowrank=True, adapter_gating_down_dim=96,
        use_encoder_adapter_gating_add=False, use_encoder_adapter_gating_small_xy_cat=False,
        use_encoder_adapter_gating_middle_xy_add=False, use_encoder_adapter_gating_middle_ia3_add=False,
        use_encoder_gating_scaling=False, encoder_gating_scaling_factor=1.0,
        use_encoder_adapter_scaling=False, encoder_adapter_scaling_factor=1.0,
        use_encoder_x2_scaling=False, encoder_x2_scaling_factor=1.0,
        unfreeze_encoder_layer_norms=True, unfreeze_layer_norms=False, unfreeze_bias=False,
        use_decoder_enc_attn_value_parallel_adapter_down_dim=True, decoder_enc_attn_value_parallel_adapter_down_dim=96,
        use_decoder_enc_attn_value_parallel_adapter_scaling=False,
        decoder_enc_attn_value_parallel_adapter_scaling_factor=1.0,
        use_lora=False, lora_dim=4, lora_alpha=32, lora_dropout=0.1, use_single_lora=False, reduction_factor=8,
        use_encoder_multihead_up_zero_init=False, use_encoder_gating_large_x_lowrank_up_zero_init=False,
        use_decoder_enc_vpa_up_zero_init=False, freeze_vis_emb=False,
        **COMPACTER_DEFAULTS, **PROMPT_DEFAULTS, **HYPERFORMER_DEFAULTS,
    )
    for k, v in over.items():
        if not hasattr(c, k):
            raise AttributeError(f"unknown config field {k}")
        setattr(c, k, v)
    check_sequential_adapter_flags(c)
    task_list = [t for t in c.tasks.replace(" ", ",").split(",") if t]
    c.task_list = task_list
    c.encoder_prompt_config = make_prompt_config(c, task_list)
    if c.use_adapter or c.use_compacter or c.use_hyperformer or c.use_decoder_enc_attn_value_parallel_adapter_down_dim:
        c.adapter_config = make_adapter_config(c, task_list)
    else:
        c.adapter_config = None
    c.lora_config = LoraConfig(lora_dim=c.lora_dim, lora_alpha=c.lora_alpha, lora_dropout=c.lora_dropout,
                               tasks=task_list, use_single_lora=c.use_single_lora) if c.use_lora else None
    return c


class HostLayerNorm(nn.LayerNorm):
    """LayerNorm whose (possibly fp32, trainable) affine parameters follow the activation dtype."""

    def forward(self, x):
        w, b = self.weight, self.bias       # (LoRA runs train every bias but no LayerNorm weight: the two may differ in dtype)
        if w.dtype != x.dtype:
            w = w.to(x.dtype)
        if b is not None and b.dtype != x.dtype:
            b = b.to(x.dtype)
        return F.layer_norm(x, self.normalized_shape, w, b, self.eps)


# K1's gate and the sublayer tail both read the sublayer input; with a link the tail's backward hands its d/dx1 to K1's
# backward kernel instead of leaving the sum to an elementwise pass of autograd (functional.ResidualLink).  The CPU parity
# harness of the test suite switches it off: its ops are plain autograd.
FUSE_RESIDUAL_GRAD = True      # (A/B switch, tools/ab_switches.py: False = plain autograd sums)


def _pet_then_tail(layer, which, residual, h, norm, p, training, config, gemm_link=None):
    """``norm(residual + dropout(apply_pet(residual, h)))`` -- K1 followed by K5.  ``gemm_link``: the link the sublayer's first
    projection armed (_first_linear): K1's d/dresidual (which already holds the tail's) goes out through it."""
    if not FUSE_RESIDUAL_GRAD:
        return sublayer_tail(residual, apply_pet(layer, which, residual, h, config), norm, p, training)
    link = VF.ResidualLink()
    y = apply_pet(layer, which, residual, h, config, link=link, out_link=gemm_link)
    return sublayer_tail(residual, y, norm, p, training, link=link)


# Sequential adapters (the Single-Adapter baseline: ``attn_adapter`` / ``ff_adapter`` of the encoder layers, ``self_attn_adapter`` /
# ``enc_attn_adapter`` / ``ff_adapter`` of the decoder layers) sit between the sublayer and its tail.  Where no gradient and no dropout
# is needed and the shape is one the kernel takes, adapter + residual + LayerNorm are ONE launch (vlpet_amd.adapter_tail); everywhere
# else K2 (x and residual the same tensor) followed by K5.
FUSE_ADAPTER_TAIL = True     # (A/B switch, tools/ab_switches.py: False = always K2 + K5)


def _adapter_then_tail(ctl, task, residual, h, norm, p, training, gemm_link=None):
    """``norm(residual + dropout(h + s * adapter(h)))`` -- my_transformers/modeling_bart.py:1145-1146 + :1259-1261 (encoder),
    :1660-1661, 1717-1718, 1759-1760 (decoder)"""
    ad = fused_adapter_tail(FUSE_ADAPTER_TAIL, ctl, task, h, residual, norm, p, training)
    if ad is not None:
        scale = float(ctl.config.scaling_factor) if ctl.config.use_scaling_factor else 1.0
        return AT.adapter_tail(h, residual, *ad.tail_weights(), norm, scale)
    return _tail_linked(residual, ctl(h, task), norm, p, training, gemm_link)


def _generated_then_tail(meta, w, residual, h, norm, p, training, gemm_link=None):
    """``_adapter_then_tail`` for Hyperformer: the adapter's weights ``w`` (adapters.AdapterWeights) were generated by the stack's
    hyper-network -- my_transformers/modeling_bart.py:1253-1254, 1369-1370 (encoder), :1674-1675, 1738-1739, 1773-1774 (decoder)"""
    if fused_generated_tail(FUSE_ADAPTER_TAIL, meta, w, h, residual, norm, p, training):
        return AT.adapter_tail(h, residual, *w.tail_weights(), norm, 1.0)
    return _tail_linked(residual, meta.fused(h, h, w), norm, p, training, gemm_link)


# The same hand-over one op further: the input of a sublayer is also the input of its first frozen projection (q|k|v, q_proj,
# fc1), whose dgrad GEMM accumulates onto the gradient K1 / the tail parked (functional.linear_acc: beta = 1 in the GEMM
# epilogue) instead of autograd adding two [M, d] tensors; in the cross-attention, k_proj / v_proj and the value-parallel
# adapter (K2) all read the encoder output: one gradient per decoder layer instead of three.
FUSE_GEMM_GRAD = True       # (A/B switch, tools/ab_switches.py: False = autograd's adds)


def _frozen(*mods) -> bool:
    return all(isinstance(m, nn.Linear) for m in mods) and not any(
        t is not None and t.requires_grad for m in mods for t in (m.weight, m.bias))


def _new_gemm_link(x):
    """A link for the first projection of a sublayer whose input is ``x``, or None when nothing would use it."""
    if not (FUSE_RESIDUAL_GRAD and FUSE_GEMM_GRAD) or not x.requires_grad or not torch.is_grad_enabled():
        return None
    return VF.ResidualLink()


def _first_linear(mod, x, link):
    """``mod(x)`` for the first projection of a sublayer; with a link and a frozen ``nn.Linear``: functional.linear_acc."""
    if link is not None and _frozen(mod):
        return VF.linear_acc(x, link, mod)
    if (link is not None and FUSE_BIAS_GRAD and isinstance(mod, nn.Linear) and not mod.weight.requires_grad and mod.bias is not None
            and mod.bias.requires_grad):
        # frozen weight, trainable bias (the LoRA runs): the same hand-over through the bias-gradient form of the projection
        w = mod.weight if mod.weight.dtype == x.dtype else mod.weight.to(x.dtype)
        if VF.linear_train_bias_ok(x, w, mod.bias):
            return VF.linear_train_bias(x, w, mod.bias, link)
    return _linear(mod, x)


def sublayer_tail(residual, h, norm, p, training, link=None):
    """K5: ``norm(residual + dropout(h))`` -- one fused HIP pass (vlpet_amd.tail); the parity / CPU-baseline harnesses
    swap this module attribute for an eager restatement."""
    from ..tail import sublayer_tail as _hip_tail
    return _hip_tail(residual, h, norm, p, training, link=link)


def _tail_linked(residual, h, norm, p, training, link):
    """K5 whose d/dresidual goes to the sublayer's first dgrad GEMM when that armed ``link`` (the swapped-in eager tail of
    the parity harness takes no link: it is only ever called without one)."""
    link = VF.ResidualLink.if_armed(link)
    if link is None:
        return sublayer_tail(residual, h, norm, p, training)
    return sublayer_tail(residual, h, norm, p, training, link=link)


def _ffn_in(fc1, x, link, act, p, training, sites=True):
    """``ffn_activation(fc1(x))`` of a feed-forward sublayer.  BitFit (frozen weight, trainable bias): one autograd pair whose backward
    sums the bias gradient inside the activation backward (act.linear_act_dropout); else _first_linear + ffn_activation.  ``sites``:
    False keeps a flag set on the path it always took (the LoRA runs, which also train every bias)."""
    # (a harness that swapped ``ffn_activation`` for its own restatement keeps it: the site replaces the HIP pass only)
    if (sites and not EAGER_FFN_ACT and ffn_activation is _HIP_FFN_ACTIVATION and isinstance(fc1, nn.Linear) and fc1.bias is not None
            and fc1.bias.requires_grad and not fc1.weight.requires_grad and torch.is_grad_enabled() and VF.FUSE_BIAS_GRAD_SITES
            and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32)):
        from ..act import linear_act_dropout, linear_act_dropout_ok
        if linear_act_dropout_ok(x, fc1, act):
            return linear_act_dropout(x, fc1, act, p, training, link)
        VF.BITFIT_CALLS["fallback"] += 1            # eligible by device and dtype, refused by shape
    return ffn_activation(_first_linear(fc1, x, link), act, p, training)


def ffn_activation(x, act, p, training):
    """``dropout(act(fc1 output), p)`` of the feed-forward sublayer: one fused HIP pass (vlpet_amd.act); the parity /
    CPU-baseline harnesses swap this module attribute for the eager pair."""
    if EAGER_FFN_ACT:
        return F.dropout(F.gelu(x) if act == "gelu" else F.relu(x), p=p, training=training)
    from ..act import act_dropout
    return act_dropout(x, act, p, training)


EAGER_FFN_ACT = False     # A/B switch (tools/ab_switches.py): the two elementwise torch passes instead
_HIP_FFN_ACTIVATION = ffn_activation


def lm_loss(h, weight, labels, bias=None):
    """LM head + per-token cross entropy (vlpet_amd.lmloss: library GEMM, then one fused HIP pass each way over the
    logits); the parity / CPU-baseline harnesses swap this module attribute for the eager chain."""
    if EAGER_LM_LOSS:
        logits = F.linear(h, weight.to(h.dtype))
        if bias is not None:
            logits = logits + bias.to(h.dtype)
        loss = F.cross_entropy(logits.float().view(-1, logits.shape[-1]), labels.view(-1), ignore_index=-100, reduction="none")
        return loss.view(labels.shape), logits
    from ..lmloss import lm_head_loss
    return lm_head_loss(h, weight, labels, bias)


EAGER_LM_LOSS = False       # A/B switch (tools/ab_switches.py): torch's cast + log_softmax + nll chain


def _linear(mod: nn.Linear, x):
    w, b = mod.weight, mod.bias             # (a trainable fp32 bias next to a frozen bf16 weight in LoRA runs)
    if w.dtype != x.dtype:
        w = w.to(x.dtype)
    if FUSE_BIAS_GRAD and b is not None and b.requires_grad:
        if VF.linear_train_bias_ok(x, w, b):
            return VF.linear_train_bias(x, w, b)             # bias gradient = column sums of dy on the HIP path
    if b is not None and b.dtype != x.dtype:
        b = b.to(x.dtype)
    return F.linear(x, w, b)


def _sdpa_ctx():
    """Frozen-backbone attention = torch SDPA with its default backend choice; ``SDPA_BACKEND`` = flash | efficient | math pins
    one (an experiment switch for the host model, not part of the PET path)."""
    import contextlib
    which = SDPA_BACKEND
    if not which:
        return contextlib.nullcontext()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    return sdpa_kernel({"flash": SDPBackend.FLASH_ATTENTION, "efficient": SDPBackend.EFFICIENT_ATTENTION,
                        "math": SDPBackend.MATH}[which])


def attention_core(q, k, v, num_heads, attn_mask, causal, p, training, k_slot=None):
    """``dropout(softmax(q k^T / sqrt(d) + mask), p) v`` on the projection outputs ``[B, L, H * d]``.  Sequences of at most
    128 tokens in bf16 with head dim 64 (every image-text shape) run on vlpet_amd.attention's on-chip kernels; anything
    else (fp32 parity runs, the 664-token video encoder, non-boolean masks) on torch's SDPA -- or, up to 1,024 tokens, on the long
    kernels where ``attention.route`` says so under this module's switches.  The parity / CPU-baseline harnesses swap this module
    attribute for the eager chain."""
    B, Lq, E = q.shape
    kind = _route(Lq, k.shape[1], p, training, q, k, v) if attn_mask is None or is_key_mask(attn_mask) else None
    if A.fits(kind, q, k, v, num_heads):
        km = None if attn_mask is None else attn_mask[:, 0, 0, :]
        return A.attend(kind, q, k, v, num_heads, km, causal and attn_mask is None, p, training, k_slot=k_slot)
    sh = lambda t: t.reshape(B, -1, num_heads, E // num_heads).transpose(1, 2)
    with _sdpa_ctx():
        out = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=attn_mask, is_causal=causal and attn_mask is None,
                                             dropout_p=p if training else 0.0)
    return out.transpose(1, 2).reshape(B, Lq, E)


FUSE_BIAS_GRAD = True    # A/B switch (tools/ab_switches.py): False = autograd's sum(0) for trainable biases
EAGER_ATTENTION = False   # A/B switch: the library (SDPA) path for every shape
LONG_ATTENTION = False    # switch: True = sequences of 129 .. 1,024 tokens (the 664-token video encoder) run on vlpet_amd.attention's
                          # forward-only long kernel wherever no dropout and no gradient is needed: a bitwise reproducible encoder
LONG_ATTENTION_TRAIN = False   # switch: True = the same lengths on the long TRAINING kernels (dropout by the device generator, a backward
                               # with a fixed summation order) wherever a call needs dropout or a gradient


def _route(Lq, Lk, p, training, *tensors, grad=False):
    """attention.route under this module's switches (``grad``: the caller knows of a gradient that the tensors do not show)"""
    return A.route(Lq, Lk, p, training, A.needs_grad(*tensors, grad=grad), eager=EAGER_ATTENTION, long_on=LONG_ATTENTION,
                   long_train_on=LONG_ATTENTION_TRAIN)


def _long_applies(Lq, Lk, p, training, *tensors) -> bool:
    return _route(Lq, Lk, p, training, *tensors) == "long"


def _long_train_applies(Lq, Lk, p, training, *tensors, grad=False) -> bool:
    return _route(Lq, Lk, p, training, *tensors, grad=grad) == "long_train"
FUSE_QKV = True              # A/B switch: False = separate q / k / v projections in self-attention
FUSE_CROSS_KEYS = True       # A/B switch: False = every decoder layer projects its own cross-attention keys (round 5)
SDPA_BACKEND = None          # A/B switch: "flash" | "efficient" | "math" pins torch SDPA's backend on the library path


class BartAttention(nn.Module):
    """Multi-head attention; optional LoRA on q/v (my_transformers/modeling_bart.py:738-879) and optional
    value-parallel adapter on the cross-attention value (:283-566, use at :427-430)."""

    def __init__(self, config, embed_dim, num_heads, dropout, is_cross=False, value_adapter=False):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.head_dim = embed_dim // num_heads
        self.use_lora = bool(config.use_lora)
        if self.use_lora:
            self.q_proj = LoRALinearController(embed_dim, embed_dim, config=config.lora_config, bias=True)
            self.v_proj = LoRALinearController(embed_dim, embed_dim, config=config.lora_config, bias=True)
        else:
            self.q_proj = nn.Linear(embed_dim, embed_dim)
            self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.attn_value_parallel_adapter = None
        if value_adapter:
            self.attn_value_parallel_adapter = value_parallel_adapter(config)

    def _shape(self, t, B):
        return t.view(B, -1, self.num_heads, self.head_dim).transpose(1, 2)

    def _fused_qkv(self, dtype):
        """The frozen q | k | v projections of a self-attention as one [3E, E] weight and [3E] bias (common.derived_weights)"""
        return derived_weights(self, "_qkv_cache", (self.q_proj, self.k_proj, self.v_proj), dtype)

    def forward(self, hidden, kv=None, attn_mask=None, causal=False, task=None, in_link=None, k_pre=None):
        """``in_link``: see _first_linear -- armed by the projection of ``hidden`` (q|k|v or q_proj) when that is frozen.
        ``k_pre`` = (k, k_slot): this layer's keys already projected (cross-attention: a column block of the decoder's fused key
        projection of the encoder output, BartDecoder._cross_keys)."""
        B, L, _ = hidden.shape
        src = hidden if kv is None else kv
        if kv is None and FUSE_QKV and not self.use_lora and not EAGER_ATTENTION:
            # self-attention with frozen projections: one [E -> 3E] GEMM each way, the attention kernels read / write the
            # q | k | v column blocks in place (one input gradient instead of three that autograd would have to sum)
            qkv_mods = (self.q_proj, self.k_proj, self.v_proj)
            frozen = not any(t.requires_grad for m in qkv_mods for t in (m.weight, m.bias))
            # BitFit: frozen weights, any subset of the three biases trainable -- the same fused GEMM, the bias gradients as one segmented
            # column sum of the fused dy (functional.linear_acc_bias)
            only_biases = not frozen and not any(m.weight.requires_grad for m in qkv_mods) and VF.FUSE_BIAS_GRAD_SITES
            bias_sites = only_biases and torch.is_grad_enabled()
            if only_biases and not bias_sites:      # evaluation of such a model (no_grad): nothing trains here, the fused bias is current
                frozen = True                       # (host.common.derived_weights keys it on the optimizer's epoch)
            kind = _route(L, L, self.dropout, self.training, hidden, grad=in_link is not None or bias_sites)
            if ((frozen or bias_sites) and (attn_mask is None or is_key_mask(attn_mask)) and hidden.is_cuda and hidden.dtype == torch.bfloat16
                    and kind is not None and self.head_dim == A.HEAD_DIM):
                w, b = self._fused_qkv(hidden.dtype)
                biases = tuple(m.bias for m in qkv_mods)
                if bias_sites and VF.linear_acc_bias_ok(hidden, w, biases):
                    qkv = VF.linear_acc_bias(hidden, in_link, w, b, biases)     # (``b`` is keyed on the optimizer's epoch: derived_weights)
                elif bias_sites:
                    VF.BITFIT_CALLS["fallback"] += 1
                    qkv = None
                elif in_link is not None:
                    qkv = VF.linear_acc(hidden, in_link, (w, b))
                else:
                    qkv = F.linear(hidden, w, b)
                if qkv is not None:
                    km = None if attn_mask is None else attn_mask[:, 0, 0, :]
                    out = A.attend_qkv(kind, qkv, self.num_heads, km, causal and attn_mask is None, self.dropout, self.training)
                    return _linear(self.out_proj, out)
        if self.use_lora:
            q = self.q_proj(hidden, task)
            v = self.v_proj(src, task)
            k = _linear(self.k_proj, src)
        else:
            # (self-attention off the fused path: hidden feeds three projections -- only q_proj takes the sublayer's link)
            q = _first_linear(self.q_proj, hidden, in_link)
            kv_frozen = kv is not None and _frozen(self.k_proj, self.v_proj)
            # BitFit: frozen weights, trainable biases -- the same single input gradient, each bias summed from its own dy
            kv_bias = kv is not None and not kv_frozen and VF.linear_acc_sep_bias_ok(src, self.k_proj, self.v_proj)
            kv_link = _new_gemm_link(src) if (kv_frozen or kv_bias) else None
            if kv_link is not None:
                acc = VF.linear_acc_sep_bias if kv_bias else VF.linear_acc
                k_slot = None
                if k_pre is not None:
                    (k, k_slot), v = k_pre, acc(src, kv_link, self.v_proj)
                else:
                    k, v = acc(src, kv_link, self.k_proj, self.v_proj)      # one gradient for the encoder output, K2's included
                if self.attn_value_parallel_adapter is not None:
                    v = self.attn_value_parallel_adapter(src, task, y=v, link=kv_link)
                out = attention_core(q, k, v, self.num_heads, attn_mask, causal, self.dropout, self.training, k_slot=k_slot)
                return _linear(self.out_proj, out)
            v = _linear(self.v_proj, src)
            k = _linear(self.k_proj, src)
        if kv is not None and self.attn_value_parallel_adapter is not None:
            v = self.attn_value_parallel_adapter(src, task, y=v)
        out = attention_core(q, k, v, self.num_heads, attn_mask, causal, self.dropout, self.training)
        return _linear(self.out_proj, out)


    # ---- generate(): one decoder token against the caches (decode.decode_attention; the same projections as forward)
    def _step_qkv(self, x, task):
        """q, k, v rows [B, E] of one token x [B, 1, E]: the fused q|k|v GEMM (column blocks read in place), or the LoRA q / v path"""
        if self.use_lora:
            return self.q_proj(x, task)[:, 0], _linear(self.k_proj, x)[:, 0], self.v_proj(x, task)[:, 0]
        if FUSE_QKV:
            w, b = self._fused_qkv(x.dtype)
            qkv = F.linear(x[:, 0], w, b)
            E = self.embed_dim
            return qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        return _linear(self.q_proj, x)[:, 0], _linear(self.k_proj, x)[:, 0], _linear(self.v_proj, x)[:, 0]

    def step_self(self, x, k_cache, v_cache, pos, task=None, key_rows=None, pos_dev=None):
        """causal self-attention of the token at ``pos``: its key / value rows go into cache row ``pos`` inside the attention launch
        (beam search: earlier keys are looked up through ``key_rows``).  ``pos_dev``: the position word instead of ``pos``,
        ``key_rows`` then both ping-pong halves (decode.decode_attention)"""
        q, k, v = self._step_qkv(x, task)
        out = D.decode_attention(q, k_cache, v_cache, self.num_heads, pos=pos, k_new=k, v_new=v, scale=self.head_dim ** -0.5,
                                 key_rows=key_rows, pos_dev=pos_dev)
        return _linear(self.out_proj, out[:, None])

    def cross_values(self, enc, task=None):
        """the cross-attention value cache: v_proj(enc) (K3 under LoRA), the value-parallel adapter (K2) applied once -- the reference
        skips K2 on cached steps because the value it feeds is cached (my_transformers/modeling_bart.py:419-430)"""
        v = self.v_proj(enc, task) if self.use_lora else _linear(self.v_proj, enc)
        if self.attn_value_parallel_adapter is not None:
            v = self.attn_value_parallel_adapter(enc, task, y=v)
        return v

    def step_cross(self, x, k_cache, v_cache, key_mask, task=None, group=1):
        q = self.q_proj(x, task) if self.use_lora else _linear(self.q_proj, x)
        out = D.decode_attention(q[:, 0], k_cache, v_cache, self.num_heads, key_mask=key_mask, scale=self.head_dim ** -0.5,
                                 group=group)
        return _linear(self.out_proj, out[:, None])


class BartEncoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        d = config.d_model
        self.embed_dim = d
        self.self_attn = BartAttention(config, d, config.encoder_attention_heads, config.attention_dropout)
        self.self_attn_layer_norm = HostLayerNorm(d)
        self.dropout, self.activation_dropout = config.dropout, config.activation_dropout
        self.fc1 = nn.Linear(d, config.encoder_ffn_dim)
        self.fc2 = nn.Linear(config.encoder_ffn_dim, d)
        self.final_layer_norm = HostLayerNorm(d)
        build_pet(self, config, d, ("attn", "ff"))
        # my_transformers/modeling_bart.py:932-947: one AdapterController behind the attention, one behind fc2
        self.attn_adapter = self.ff_adapter = None
        if sequential_adapters(config, "encoder"):
            self.attn_adapter = AdapterController(config.adapter_config)
            self.ff_adapter = AdapterController(config.adapter_config)
        self.adapter_hypernet = MetaLayersAdapterController(config.adapter_config) if hyperformer(config) else None      # (:949-951)
        # the reference's BART encoder layer has no adapter / x2 scaling (my_transformers/modeling_bart.py:1147-1155 is a plain
        # h + up(...)); only the T5 layers read those flags (my_transformers/modeling_t5.py:373-377, 789-793)
        self.pet_config = copy.copy(config)
        self.pet_config.use_encoder_adapter_scaling = False
        self.pet_config.use_encoder_x2_scaling = False

    def forward(self, hidden, attn_mask=None, task=None, block_adapters=None):
        residual = hidden
        gl = _new_gemm_link(hidden)
        h = self.self_attn(hidden, attn_mask=attn_mask, task=task, in_link=gl)
        if self.adapter_hypernet is not None:                                       # generated adapter: K2 + K5 | the fused launch
            hidden = _generated_then_tail(self.adapter_hypernet, block_adapters["self_attention"], residual, h, self.self_attn_layer_norm,
                                          self.dropout, self.training, gl)
        elif self.attn_adapter is not None:                                           # K2 + K5 | the fused launch
            hidden = _adapter_then_tail(self.attn_adapter, task, residual, h, self.self_attn_layer_norm, self.dropout, self.training, gl)
        elif has_pet(self, "attn"):                                                 # K1 + K5
            hidden = _pet_then_tail(self, "attn", residual, h, self.self_attn_layer_norm, self.dropout, self.training,
                                    self.pet_config, gemm_link=gl)
        else:
            hidden = _tail_linked(residual, h, self.self_attn_layer_norm, self.dropout, self.training, gl)   # K5
        residual = hidden
        gl = _new_gemm_link(hidden)
        h = _ffn_in(self.fc1, hidden, gl, "gelu", self.activation_dropout, self.training, sites=not self.config.use_lora)
        h = _linear(self.fc2, h)
        if self.adapter_hypernet is not None:
            return _generated_then_tail(self.adapter_hypernet, block_adapters["feed_forward"], residual, h, self.final_layer_norm,
                                        self.dropout, self.training, gl)
        if self.ff_adapter is not None:
            return _adapter_then_tail(self.ff_adapter, task, residual, h, self.final_layer_norm, self.dropout, self.training, gl)
        if has_pet(self, "ff"):                                                     # K1 + K5
            return _pet_then_tail(self, "ff", residual, h, self.final_layer_norm, self.dropout, self.training, self.pet_config,
                                  gemm_link=gl)
        return _tail_linked(residual, h, self.final_layer_norm, self.dropout, self.training, gl)             # K5


class BartDecoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        d = config.d_model
        self.self_attn = BartAttention(config, d, config.decoder_attention_heads, config.attention_dropout)
        self.self_attn_layer_norm = HostLayerNorm(d)
        vpa = bool(config.use_decoder_enc_attn_value_parallel_adapter_down_dim) and not config.use_lora
        self.encoder_attn = BartAttention(config, d, config.decoder_attention_heads, config.attention_dropout,
                                          is_cross=True, value_adapter=vpa)
        self.encoder_attn_layer_norm = HostLayerNorm(d)
        self.dropout, self.activation_dropout = config.dropout, config.activation_dropout
        self.fc1 = nn.Linear(d, config.decoder_ffn_dim)
        self.fc2 = nn.Linear(config.decoder_ffn_dim, d)
        self.final_layer_norm = HostLayerNorm(d)
        # my_transformers/modeling_bart.py:1525-1536: an AdapterController behind each of the three sublayers
        self.self_attn_adapter = self.enc_attn_adapter = self.ff_adapter = None
        if sequential_adapters(config, "decoder"):
            self.self_attn_adapter = AdapterController(config.adapter_config)
            if config.add_adapter_cross_attn:
                self.enc_attn_adapter = AdapterController(config.adapter_config)
            self.ff_adapter = AdapterController(config.adapter_config)
        self.adapter_hypernet = MetaLayersAdapterController(config.adapter_config) if hyperformer(config) else None      # (:1563-1565)
        self.add_adapter_cross_attn = bool(config.add_adapter_cross_attn)

    def _tail(self, ctl, task, residual, h, norm, gl=None, w=None):
        """the sublayer's tail: behind its sequential adapter when it has one; ``w``: behind the generated adapter (Hyperformer)"""
        if w is not None:
            return _generated_then_tail(self.adapter_hypernet, w, residual, h, norm, self.dropout, self.training, gl)
        if ctl is not None:
            return _adapter_then_tail(ctl, task, residual, h, norm, self.dropout, self.training, gl)
        return _tail_linked(residual, h, norm, self.dropout, self.training, gl)                            # K5

    def _generated(self, block_adapters):
        """(self-attention, cross-attention, feed-forward) generated adapters of this layer, None where there is none"""
        if self.adapter_hypernet is None:
            return None, None, None
        b = block_adapters
        return b["self_attention"], b["cross_attention"] if self.add_adapter_cross_attn else None, b["feed_forward"]

    def forward(self, hidden, enc, enc_mask=None, task=None, k_pre=None, block_adapters=None):
        ws, wx, wf = self._generated(block_adapters)
        residual = hidden
        gl = _new_gemm_link(hidden)
        h = self.self_attn(hidden, causal=True, task=task, in_link=gl)
        hidden = self._tail(self.self_attn_adapter, task, residual, h, self.self_attn_layer_norm, gl, ws)
        residual = hidden
        gl = _new_gemm_link(hidden)
        h = self.encoder_attn(hidden, kv=enc, attn_mask=enc_mask, task=task, in_link=gl, k_pre=k_pre)      # K2 inside
        hidden = self._tail(self.enc_attn_adapter, task, residual, h, self.encoder_attn_layer_norm, gl, wx)
        residual = hidden
        gl = _new_gemm_link(hidden)
        h = _ffn_in(self.fc1, hidden, gl, "gelu", self.activation_dropout, self.training, sites=not self.config.use_lora)
        h = _linear(self.fc2, h)
        return self._tail(self.ff_adapter, task, residual, h, self.final_layer_norm, gl, wf)


    def step(self, x, cache, pos, state, task=None, block_adapters=None):
        """generate(): the token x [B, 1, d] at position ``pos``; ``cache`` = this layer's (self k, self v, cross k, cross v) of
        ``state`` (decode.DecodeState)"""
        ks, vs, kx, vx = cache
        ws, wx, wf = self._generated(block_adapters)
        kr, pd = state.key_rows, state.pos_dev
        h = self.self_attn.step_self(x, ks, vs, pos, task, key_rows=kr if kr is None or pd is not None else kr[pos & 1], pos_dev=pd)
        x = self._tail(self.self_attn_adapter, task, x, h, self.self_attn_layer_norm, None, ws)             # K5 | adapter + K5 in one launch
        h = self.encoder_attn.step_cross(x, kx, vx, state.key_mask, task, group=state.group)
        x = self._tail(self.enc_attn_adapter, task, x, h, self.encoder_attn_layer_norm, None, wx)
        h = ffn_activation(_linear(self.fc1, x), "gelu", self.activation_dropout, self.training)
        return self._tail(self.ff_adapter, task, x, _linear(self.fc2, h), self.final_layer_norm, None, wf)


class LearnedPositionalEmbedding(nn.Embedding):
    """BART's learned positions with the historical offset of 2."""

    def __init__(self, num, dim):
        super().__init__(num + 2, dim)

    def forward(self, L: int, device):
        return super().forward(torch.arange(2, L + 2, device=device))


def _install_hyper_net(stack, config, task_embed, num_layers, include_cross_attention):
    """my_transformers/modeling_bart.py:1978-1987, 2144-2153: the shared TaskEmbeddingController under the stack's own name too, and the
    stack's hyper-network, registered right behind ``embed_tokens`` as there; without the flag no attribute and no state-dict key"""
    if hyperformer(config):
        stack.task_embed = task_embed
        stack.adapter_layers_hyper_net = new_hyper_net(config, num_layers, include_cross_attention)


def _stack_block_adapters(stack, task, x):
    """every layer's generated adapters for ``task`` (one generator launch), or a list of None without Hyperformer"""
    if getattr(stack, "adapter_layers_hyper_net", None) is None:
        return [None] * len(stack.layers)
    return block_adapters(stack.adapter_layers_hyper_net, stack.task_embed, task, x)


class JointEncoder(nn.Module):
    def __init__(self, config, embed_tokens, task_embed=None):
        super().__init__()
        self.config = config
        d = config.d_model
        self.dropout = config.dropout
        self.embed_scale = math.sqrt(d) if config.scale_embedding else 1.0
        self.embed_tokens = embed_tokens
        _install_hyper_net(self, config, task_embed, config.encoder_layers, False)
        self.embed_positions = LearnedPositionalEmbedding(config.max_position_embeddings, d)
        self.layers = nn.ModuleList([BartEncoderLayer(config) for _ in range(config.encoder_layers)])
        self.layernorm_embedding = HostLayerNorm(d)
        # src/modeling_bart.py:704-709: the low-rank projector replaces the full feat_dim x d_model Linear when asked for
        vis_cls = LowRankVisualEmbedding if getattr(config, "use_lowrank_visual_projector", False) else VisualEmbedding
        self.visual_embedding = vis_cls(config, self.embed_tokens)
        self.downsample = None
        if config.downsample:
            s = int(config.n_boxes ** 0.5)
            self.downsample = Downsample((s, s))
        # src/modeling_bart.py:725-728 (prompt tuning); without the flag no attribute and no state-dict key, as before
        if getattr(config, "encoder_prompt_config", None) is not None:
            self.prompt_modules = PromptController(config.encoder_prompt_config)

    def forward(self, input_ids, vis_inputs, attention_mask=None, task=None, no_padding=False):
        if getattr(self, "prompt_modules", None) is not None:
            return self._forward_prompted(input_ids, vis_inputs, attention_mask, task, no_padding)
        B, L = input_ids.shape
        if attention_mask is None and not no_padding:
            # src/modeling_bart.py:817-818: the text mask defaults to input_ids != pad; it also becomes the decoder's
            # cross-attention mask (:995-996).  ``no_padding`` = the loader's promise that no row is padded (every
            # row has the full length -- true for the synthetic batches), which keeps attention on the unmasked path
            attention_mask = input_ids.ne(self.config.pad_token_id)
        x = self.embed_tokens(input_ids) * self.embed_scale + self.embed_positions(L, input_ids.device)
        vis = self.visual_embedding(*unpack_vis_inputs(vis_inputs, self.downsample, x.dtype)).to(x.dtype)   # K4
        if self.config.share_vis_lang_layer_norm:
            x = self.layernorm_embedding(torch.cat([x, vis], dim=1))
            x = F.dropout(x, p=self.dropout, training=self.training)
        else:
            from ..act import concat_dropout
            x = concat_dropout(self.layernorm_embedding(x), vis, self.dropout, self.training)      # cat + dropout: one pass each way
        mask = None
        if attention_mask is not None:      # [B, L] text padding mask; visual tokens always attended
            full = torch.cat([attention_mask.bool(), torch.ones(B, vis.shape[1], dtype=torch.bool,
                                                                device=x.device)], dim=1)
            mask = full[:, None, None, :]
        for layer, ba in zip(self.layers, _stack_block_adapters(self, task, x)):
            x = layer(x, mask, task, ba)
        return x, mask

    def _forward_prompted(self, input_ids, vis_inputs, attention_mask, task, no_padding):
        """src/modeling_bart.py:776-833 with an encoder prompt: [prompt | text | visual].  The prompt gets no positions; it goes through
        ``layernorm_embedding`` with the text (a per-row norm: applied to its P rows once, not to B * P), and the key mask -- the
        decoder's cross-attention mask and ``generate``'s too -- is [ones(P) | text mask | ones(V)] (none under ``no_padding``)."""
        B, L = input_ids.shape
        if attention_mask is None and not no_padding:
            attention_mask = input_ids.ne(self.config.pad_token_id)
        x = self.embed_tokens(input_ids) * self.embed_scale + self.embed_positions(L, input_ids.device)
        vis = self.visual_embedding(*unpack_vis_inputs(vis_inputs, self.downsample, x.dtype)).to(x.dtype)   # K4
        pre = self.prompt_modules.prompt_rows(task).to(x.dtype)                  # [P, d]: the MLP on P rows
        P = pre.shape[0]
        if self.config.share_vis_lang_layer_norm:
            x = self.layernorm_embedding(torch.cat([pre.expand(B, -1, -1), x, vis], dim=1))
            x = F.dropout(x, p=self.dropout, training=self.training)
        else:
            from ..act import prefix_concat_dropout
            x = prefix_concat_dropout(self.layernorm_embedding(pre), self.layernorm_embedding(x), vis, self.dropout, self.training)
        mask = None
        if attention_mask is not None:
            ones = lambda n: torch.ones(B, n, dtype=torch.bool, device=x.device)
            mask = torch.cat([ones(P), attention_mask.bool(), ones(vis.shape[1])], dim=1)[:, None, None, :]
        for layer, ba in zip(self.layers, _stack_block_adapters(self, task, x)):
            x = layer(x, mask, task, ba)
        return x, mask


class BartDecoder(nn.Module):
    def __init__(self, config, embed_tokens, task_embed=None):
        super().__init__()
        d = config.d_model
        self.dropout = config.dropout
        self.embed_scale = math.sqrt(d) if config.scale_embedding else 1.0
        self.embed_tokens = embed_tokens
        _install_hyper_net(self, config, task_embed, config.decoder_layers, True)
        self.embed_positions = LearnedPositionalEmbedding(config.max_position_embeddings, d)
        self.layers = nn.ModuleList([BartDecoderLayer(config) for _ in range(config.decoder_layers)])
        self.layernorm_embedding = HostLayerNorm(d)

    def forward(self, input_ids, enc, enc_mask=None, task=None):
        B, L = input_ids.shape
        x = self.embed_tokens(input_ids) * self.embed_scale + self.embed_positions(L, input_ids.device)
        x = F.dropout(self.layernorm_embedding(x), p=self.dropout, training=self.training)
        n = len(self.layers)
        fused_keys = self._cross_keys_ok(enc, enc_mask)
        encs = VF.fanout(enc, n + (1 if fused_keys else 0))        # one gradient sum for the encoder output instead of autograd's pairwise adds
        ks = self._cross_keys(encs[n]) if fused_keys else None
        bas = _stack_block_adapters(self, task, x)
        for i, (layer, e) in enumerate(zip(self.layers, encs)):
            x = layer(x, e, enc_mask, task, k_pre=None if ks is None else (ks[0][i], None if ks[1] is None else (ks[1], i)),
                      block_adapters=bas[i])
        return x

    def _cross_keys_ok(self, enc, enc_mask) -> bool:
        """The layers' cross-attention key projections as ONE GEMM (functional.cross_key_blocks): frozen plain projections, bf16 on the
        GPU, a shape the short-sequence attention kernels take (they read a layer's keys as a column block in place)."""
        if not FUSE_CROSS_KEYS or EAGER_ATTENTION or len(self.layers) < 2 or not enc.is_cuda or enc.dtype != torch.bfloat16:
            return False
        a0 = self.layers[0].encoder_attn
        # (past the short kernels' length the forward-only long kernel reads a column block in place, and so do the long training kernels,
        # which also write dk into the shared slot; any gradient mode counts as a gradient needed: the queries are not known here)
        if _route(enc.shape[1], enc.shape[1], a0.dropout, self.training, grad=True) is None or a0.head_dim != A.HEAD_DIM:
            return False
        if enc_mask is not None and not is_key_mask(enc_mask):
            return False
        def ok(a):          # frozen plain projections -- or (BitFit) frozen weights with trainable biases, whose gradients the fused form sums
            return not a.use_lora and (_frozen(a.k_proj, a.v_proj) or VF.linear_acc_sep_bias_ok(enc, a.k_proj, a.v_proj))
        return all(ok(l.encoder_attn) for l in self.layers)

    def _cross_keys(self, enc):
        mods = [l.encoder_attn.k_proj for l in self.layers]
        w, b = derived_weights(self, "_ck_cache", mods, enc.dtype)
        return VF.cross_key_blocks(enc, w, b, len(mods), [m.bias for m in mods])


    def init_cache(self, enc, key_mask, task, max_length, num_beams=1):
        """generate(): the decode.DecodeState of a call over ``enc``: the cross-attention keys as column blocks of ONE fused
        projection where the layers allow it, the values through K2 / K3 once; ``num_beams`` K > 1: self-attention caches of B * K
        rows, the cross-attention ones stay per item."""
        if FUSE_CROSS_KEYS and not EAGER_ATTENTION and len(self.layers) >= 2 and enc.is_cuda:
            ks = self._cross_keys(enc)[0]
        else:
            ks = [_linear(l.encoder_attn.k_proj, enc) for l in self.layers]
        vs = [l.encoder_attn.cross_values(enc, task) for l in self.layers]
        return D.new_decode_state(enc, enc.shape[2], max_length, ks, vs, key_mask, num_beams)

    def block_adapters(self, task, x):
        """generate(): every layer's generated adapters for ``task``, once per call -- under no_grad they are the controller's cached
        buffers of that task, refreshed in place, so a captured step keeps reading valid memory"""
        return _stack_block_adapters(self, task, x)

    def step(self, tok, pos, state, task=None, block_adapters=None):
        """generate(): hidden state [B, d] of the tokens ``tok`` [B] at position ``pos`` (learned position pos + 2); with
        ``state.pos_dev`` the position is the device word's (a gather) and ``pos`` is not read"""
        if state.pos_dev is not None:
            p = self.embed_positions.weight[2:].index_select(0, state.pos_dev)
        else:
            p = self.embed_positions.weight[pos + 2]
        x = self.embed_tokens(tok)[:, None] * self.embed_scale + p
        x = F.dropout(self.layernorm_embedding(x), p=self.dropout, training=self.training)
        bas = block_adapters if block_adapters is not None else [None] * len(self.layers)
        for layer, c, ba in zip(self.layers, state.layers, bas):
            x = layer.step(x, c, pos, state, task, ba)
        return x[:, 0]


class VLBartModel(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.shared = nn.Embedding(config.vocab_size, config.d_model, padding_idx=config.pad_token_id)
        # src/modeling_bart.py:1303-1313: ONE TaskEmbeddingController, registered here and under both stacks
        task_embed = None           # (without the flag no attribute at all: the module tree of every other flag set is unchanged)
        if hyperformer(config):
            self.shared_task_embed = task_embed = TaskEmbeddingController(config.adapter_config)
        self.encoder = JointEncoder(config, self.shared, task_embed)
        self.decoder = BartDecoder(config, self.shared, task_embed)


shift_tokens_right = shift_right


class VLBart(nn.Module):
    """Encoder-decoder + tied LM head; ``forward`` returns the per-token loss [B, L] like the
    reference's ``reduce_loss=False`` path (src/modeling_bart.py:1574-1586)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.model = VLBartModel(config)
        self.register_buffer("final_logits_bias", torch.zeros(1, config.vocab_size))
        install_shared_phm_rule(self, [self.model], config.adapter_config)        # (Compacter with shared_phm_rule)
        self.apply(self._init_weights)
        # derived copies of frozen tensors (fused q|k|v, padded LM head, fp32 norms) must not outlive a checkpoint load
        self.register_load_state_dict_post_hook(lambda module, incompatible: VF.invalidate_caches())

    def _init_weights(self, m):
        # my_transformers/modeling_bart.py:1819-1828: every Linear (adapters included) ~ N(0, 0.02), zero bias
        std = self.config.init_std
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(0.0, std)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(0.0, std)
            if m.padding_idx is not None:
                m.weight.data[m.padding_idx].zero_()
        if isinstance(m, LoRALinearController):
            for t in m.tasks:
                nn.init.zeros_(m.lora_Bs[t])

    def _logits_bias(self):
        """final_logits_bias (src/modeling_bart.py:1470, 1574) is a zero buffer unless a checkpoint carries one: checked once
        per buffer version (one host sync), so the usual all-zero case adds no pass over the logits."""
        b = self.final_logits_bias
        key = (b.data_ptr(), b._version, VF.FROZEN_EPOCH)
        if getattr(self, "_bias_key", None) != key:
            self._bias_key, self._bias_nonzero = key, bool(b.any())
        return b if self._bias_nonzero else None

    def forward(self, input_ids, vis_inputs, labels, task, attention_mask=None, no_padding=False):
        cfg = self.config
        enc, mask = self.model.encoder(input_ids, vis_inputs, attention_mask, task, no_padding)
        dec_in = shift_tokens_right(labels, cfg.pad_token_id, cfg.decoder_start_token_id)
        h = self.model.decoder(dec_in, enc, mask, task)
        return lm_loss(h, self.model.shared.weight, labels, self._logits_bias())

    def generate(self, input_ids, vis_inputs, task, attention_mask=None, max_length=20, min_length=0, no_repeat_ngram_size=0,
                 eos_token_id=None, pad_token_id=None, no_padding=False, num_beams=1, length_penalty=1.0, early_stopping=False,
                 graph=False):
        """Greedy search with HF 4.2.1 semantics (num_beams = 1; the reference's evaluation, src/multitask.py test_step) on a per-layer
        key / value cache: the encoder runs once, every step feeds one token (vlpet_amd.decode).  Returns the token ids
        [B, <= max_length], starting with decoder_start_token_id; finished rows are padded.  eos / pad default to the config's
        (BART: 2 / 1).  Pass the checkpoint's own generation settings (min_length, no_repeat_ngram_size) explicitly.
        ``num_beams`` > 1: HF 4.2.1 beam search (one sequence per item; the video captioning evaluation, src/multitask_video.py)
        with ``length_penalty`` / ``early_stopping``, BART's forced eos at the last step, and the cross-attention caches kept per
        item (decode.beam_generate, which also returns each sequence's score).
        ``graph=True``: the decode step is captured once per shape and replayed (decode.graph_generate: the first call of a shape
        runs eagerly, the second captures); CPU tensors and inputs the decode kernels do not take run the plain loop."""
        from ..lmloss import _padded_head
        cfg = self.config
        eos = getattr(cfg, "eos_token_id", 2) if eos_token_id is None else eos_token_id
        pad = cfg.pad_token_id if pad_token_id is None else pad_token_id
        with eval_no_grad(self):
            enc, mask = self.model.encoder(input_ids, vis_inputs, attention_mask, task, no_padding)
            key_mask = None if mask is None else mask[:, 0, 0, :].contiguous()
            dec = self.model.decoder
            state = dec.init_cache(enc, key_mask, task, max_length, num_beams=int(num_beams))
            bas = dec.block_adapters(task, enc)
            V = self.model.shared.weight.shape[0]
            head = _padded_head(self.model.shared.weight, enc.dtype)
            bias = self._logits_bias()

            def make_step(st):
                def step(tok, pos):
                    logits = F.linear(dec.step(tok, pos, st, task, bas), head)
                    if bias is not None:
                        logits[:, :V] += bias[0].to(logits.dtype)
                    return logits
                return step
            if graph:
                gs = D.GenSettings(cfg.decoder_start_token_id, eos, int(pad), int(max_length), int(min_length),
                                   int(no_repeat_ngram_size), int(num_beams), float(length_penalty), bool(early_stopping), True)
                return D.graph_generate(self, state, make_step, V, cfg.decoder_attention_heads, head, gs, key_extra=(task,))[0]
            return D.generate(make_step(state), V, enc.shape[0], enc.device, state.key_rows, cfg.decoder_start_token_id, eos, pad,
                              max_length, min_length, no_repeat_ngram_size, int(num_beams), length_penalty, early_stopping,
                              force_eos=True)
