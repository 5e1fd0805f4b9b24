"""Minimal VL-T5 host (frozen T5 encoder-decoder in plain PyTorch-ROCm: relative-position attention, RMS
norms, ReLU feed-forward), no HIP code of ours -- the PET arithmetic is delegated to ``encoder_pet.apply_pet``
(K1, with the T5-only delta / x2 / gate scaling factors), ``adapters.AdapterController`` (K2 on the
cross-attention value), ``visual.VisualEmbedding`` (K4, RMS-norm form) and ``tail.sublayer_tail`` (K5 without a
norm: T5 is pre-LN, the tail is ``hidden + dropout(y)``).

Mirrors, with the reference's parameter names (state-dict compatible):
  my_transformers/modeling_t5.py:288-410 (T5LayerFF + inline adapter/gate), :412-678 (T5Attention incl.
  ``project_vpa``), :679-827 (T5LayerSelfAttention + inline adapter/gate), :829-894 (T5LayerCrossAttention),
  :896-1000 (T5Block), :1090-1458 (T5Stack);  src/modeling_t5.py:176-405 (JointEncoder: [text ; visual] order,
  relative-position bias only inside the text block), :407-700 (VLT5: tied head rescaled by d_model**-0.5).
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
from ..visual import Downsample, T5LayerNorm, VisualEmbedding
from ..prompt import PromptController
from .bart import TASKS, _linear
from .common import (COMPACTER_DEFAULTS, HYPERFORMER_DEFAULTS, PROMPT_DEFAULTS, block_adapters, fused_generated_tail, hyperformer, new_hyper_net, check_sequential_adapter_flags, derived_weights, eval_no_grad, fused_adapter_tail,
                     install_shared_phm_rule, make_adapter_config, make_prompt_config, sequential_adapters, shift_right, unpack_vis_inputs,
                     value_parallel_adapter)


# K1's gate and the sublayer tail both read the sublayer input; with a link the tail's backward hands its d/dx1 to K1's
# backward kernel instead of leaving the sum to an elementwise pass of autograd (functional.ResidualLink).  The CPU parity
# harness of the test suite switches it off: its ops are plain autograd.
FUSE_RESIDUAL_GRAD = True      # (A/B switch, tools/ab_switches.py: False = plain autograd sums)


def _pet_then_tail(layer, which, residual, h, norm, p, training, config, norm_link=None):
    """``norm(residual + dropout(apply_pet(residual, h)))`` -- K1 followed by K5.  ``norm_link``: armed by the sublayer's RMS norm
    (which read ``residual`` first): K1's d/dresidual -- the tail's included -- goes out through it."""
    if not FUSE_RESIDUAL_GRAD:
        return sublayer_tail(residual, apply_pet(layer, which, residual, h, config), norm, p, training)
    link = VF.ResidualLink()
    y = apply_pet(layer, which, residual, h, config, link=link, out_link=norm_link)
    nxt = _fused_tail_ok(layer, y) if norm is None else None
    if nxt is not None:
        from ..tail import sublayer_tail_rms
        return sublayer_tail_rms(residual, y, nxt, p, training, link=link)
    return sublayer_tail(residual, y, norm, p, training, link=link)


# The pre-norm residual stream of a T5 sublayer is read by the RMS norm in front of it and by the tail's add behind it (and by
# K1's gate in the encoder): the later reader parks its gradient and the norm's backward kernel adds it (tail.rms_norm's link) --
# one gradient for the stream, no elementwise add by autograd (my_transformers/modeling_t5.py:366, 408; :782, 824).
FUSE_NORM_GRAD = True     # (A/B switch, tools/ab_switches.py: False = autograd's adds)


def _new_norm_link(x):
    fused = getattr(x, "_vlpet_norm", None)     # x came out of a fused tail + norm: its later readers park their gradients in THAT op's link
    if fused is not None:
        return fused.link
    if not (FUSE_RESIDUAL_GRAD and FUSE_NORM_GRAD) or not x.is_cuda or not x.requires_grad or not torch.is_grad_enabled():
        return None
    return VF.ResidualLink()


def _normed(norm, hidden, link):
    return norm(hidden) if link is None else norm(hidden, link=link)


# The sum a T5 tail produces is read next by the following sublayer's RMS norm: the tail kernel applies that norm to the row it has just
# formed and writes both (tail.sublayer_tail_rms: one pass instead of two forward, one instead of two backward).  Each sublayer module
# knows the norm that follows it (``_next_norm``, wired by ``_wire_next_norms`` when the stack is built; not a registered submodule).
FUSE_TAIL_NORM = True     # (A/B switch: False = the tail and the next norm as two launches each way)


def _fused_tail_ok(layer, y):
    nn_ = getattr(layer, "_next_norm", None)
    return (nn_[0] if (FUSE_TAIL_NORM and FUSE_RESIDUAL_GRAD and FUSE_NORM_GRAD and nn_ is not None and y.is_cuda
                       and sublayer_tail is _HIP_SUBLAYER_TAIL and y.shape[-1] % 8 == 0) else None)


def _tail_linked(hidden, y, p, training, link, layer=None):
    nxt = _fused_tail_ok(layer, y) if layer is not None else None
    link = VF.ResidualLink.if_armed(link)
    if nxt is not None:
        from ..tail import sublayer_tail_rms
        return sublayer_tail_rms(hidden, y, nxt, p, training, link=link)
    if link is None:                # (the swapped-in eager tail of the parity harness takes no link)
        return sublayer_tail(hidden, y, None, p, training)
    return sublayer_tail(hidden, y, None, p, training, link=link)


# Sequential adapters (the Single-Adapter baseline: ``attn_adapter`` / ``enc_attn_adapter`` / ``ff_adapter`` of the sublayer modules):
# ``hidden + dropout(y + s * adapter(y))`` (my_transformers/modeling_t5.py:363-364, 779-780, 886-887) is K2 (x and residual the same
# tensor) followed by the tail.  The fused launch of vlpet_amd.adapter_tail (identity norm) takes adapter + add where no gradient and
# no dropout is needed; the next sublayer's RMS norm then runs as its own kernel, so against K2 + the fused tail-and-norm pass it saves
# no launch on this host -- off by default here (host/bart.py, where it replaces two launches by one, has it on).
FUSE_ADAPTER_TAIL = False    # (A/B switch, tools/ab_switches.py)


def _adapter_then_tail(ctl, task, hidden, y, p, training, link, layer):
    ad = fused_adapter_tail(FUSE_ADAPTER_TAIL and sublayer_tail is _HIP_SUBLAYER_TAIL, ctl, task, y, hidden, None, p, training)
    if ad is not None:
        scale = float(ctl.config.scaling_factor) if ctl.config.use_scaling_factor else 1.0
        return AT.adapter_tail(y, hidden, *ad.tail_weights(), None, scale)
    return _tail_linked(hidden, ctl(y, task), p, training, link, layer=layer)


def _generated_then_tail(meta, w, hidden, y, p, training, link, layer):
    """``_adapter_then_tail`` for Hyperformer: the adapter's weights ``w`` (adapters.AdapterWeights) were generated by the stack's
    hyper-network -- my_transformers/modeling_t5.py:381-382, 797-798, 888-889"""
    if fused_generated_tail(FUSE_ADAPTER_TAIL and sublayer_tail is _HIP_SUBLAYER_TAIL, meta, w, y, hidden, None, p, training):
        return AT.adapter_tail(y, hidden, *w.tail_weights(), None, 1.0)
    return _tail_linked(hidden, meta.fused(y, y, w), p, training, link, layer=layer)


def _tail_or_adapter(ctl, task, hidden, y, p, training, link, layer, w=None):
    """the sublayer's tail: behind its sequential adapter when it has one; ``w``: behind the generated adapter (Hyperformer)"""
    if w is not None:
        return _generated_then_tail(layer.adapter_hypernet, w, hidden, y, p, training, link, layer)
    if ctl is not None:
        return _adapter_then_tail(ctl, task, hidden, y, p, training, link, layer)
    return _tail_linked(hidden, y, p, training, link, layer=layer)             # K5 (+ the next sublayer's norm)


def ffn_activation(x, act, p, training):
    """``dropout(relu(wi output))`` of T5DenseReluDense as one fused HIP pass (vlpet_amd.act); harnesses swap this
    attribute for the eager pair."""
    from ..act import act_dropout
    return act_dropout(x, act, p, training)


def lm_loss(h, weight, labels, bias=None):
    """LM head + per-token cross entropy (vlpet_amd.lmloss); harnesses swap this attribute for the eager chain."""
    from ..lmloss import lm_head_loss
    return lm_head_loss(h, weight, labels, bias)


def sublayer_tail(residual, h, norm, p, training, link=None):
    """K5 (T5 form): ``residual + dropout(h)`` -- one fused HIP pass; harnesses swap this attribute for an eager
    restatement, exactly as for host.bart."""
    from ..tail import sublayer_tail as _hip_tail
    return _hip_tail(residual, h, norm, p, training, link=link)


_HIP_SUBLAYER_TAIL = sublayer_tail      # (a parity harness that swaps ``sublayer_tail`` for an eager restatement also switches the fusion off)


def _wire_next_norms(blocks, final_norm):
    """Every sublayer module of a stack learns which T5LayerNorm reads its output: the next sublayer's, the next block's first, or
    the stack's final norm (a 1-tuple attribute, so that the norm is not registered a second time as a submodule)."""
    subs = [m for b in blocks for m in b.layer]
    for i, m in enumerate(subs):
        object.__setattr__(m, "_next_norm", ((subs[i + 1].layer_norm if i + 1 < len(subs) else final_norm),))


def vlt5_config(**over) -> SimpleNamespace:
    """t5-base + scripts/image-text/T5-VL-PET-large.sh (r = r_g = 192, decoder value adapter 96, gate scale 0.3)."""
    c = SimpleNamespace(
        d_model=768, d_kv=64, d_ff=3072, num_layers=12, num_decoder_layers=12, num_heads=12,
        relative_attention_num_buckets=32, dropout_rate=0.1, layer_norm_epsilon=1e-6, vocab_size=32100 + 100,
        pad_token_id=0, decoder_start_token_id=0, initializer_factor=1.0,
        feat_dim=2048, pos_dim=4, n_images=2, n_boxes=36, downsample=True, use_vis_order_embedding=True,
        use_vis_layer_norm=True, individual_vis_layer_norm=True, share_vis_lang_layer_norm=False,
        tasks=",".join(TASKS), use_adapter=True, use_single_adapter=True, no_encoder_adapter=True,
        no_decoder_adapter=True, add_adapter_cross_attn=True, use_adapter_down_dim=True, adapter_down_dim=192,
        use_encoder_adapter_down_multihead=True, encoder_adapter_multihead_num_head=4,
        use_encoder_adapter_gating_large_x_lowrank=True, adapter_gating_down_dim=192,
        use_encoder_adapter_gating_add=False, use_encoder_adapter_gating_small_xy_cat=False,
        use_encoder_adapter_gating_middle_xy_add=False, use_encoder_adapter_gating_middle_ia3_add=False,
        use_encoder_gating_scaling=True, encoder_gating_scaling_factor=0.3,
        use_encoder_adapter_scaling=False, encoder_adapter_scaling_factor=1.0,
        use_encoder_x2_scaling=False, encoder_x2_scaling_factor=1.0,
        unfreeze_encoder_layer_norms=True, unfreeze_layer_norms=False, unfreeze_bias=False,
        use_decoder_enc_attn_value_parallel_adapter_down_dim=True, decoder_enc_attn_value_parallel_adapter_down_dim=96,
        use_decoder_enc_attn_value_parallel_adapter_scaling=False,
        decoder_enc_attn_value_parallel_adapter_scaling_factor=1.0,
        use_lora=False, reduction_factor=8,
        use_encoder_multihead_up_zero_init=True, use_encoder_gating_large_x_lowrank_up_zero_init=True,
        use_decoder_enc_vpa_up_zero_init=True, freeze_vis_emb=False,
        **COMPACTER_DEFAULTS, **PROMPT_DEFAULTS, **HYPERFORMER_DEFAULTS,
    )
    for k, v in over.items():
        if not hasattr(c, k):
            raise AttributeError(f"unknown config field {k}")
        setattr(c, k, v)
    check_sequential_adapter_flags(c)
    c.task_list = [t for t in c.tasks.replace(" ", ",").split(",") if t]
    c.adapter_config = make_adapter_config(c, c.task_list)
    c.lora_config = None
    c.encoder_prompt_config = make_prompt_config(c, c.task_list)
    return c


def relative_position_bucket(relative_position, bidirectional, num_buckets=32, max_distance=128):
    """T5's log-spaced relative-position buckets (my_transformers/modeling_t5.py:464-507; Mesh-TensorFlow rule)."""
    buckets = torch.zeros_like(relative_position)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (relative_position > 0).long() * num_buckets
        relative_position = relative_position.abs()
    else:
        relative_position = -torch.min(relative_position, torch.zeros_like(relative_position))
    max_exact = num_buckets // 2
    small = relative_position < max_exact
    large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).long()
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(small, relative_position, large)


EAGER_ATTENTION = False   # A/B switch (tools/ab_switches.py): True = torch SDPA with a dense additive mask for every T5 attention
LONG_ATTENTION = False    # switch (host/bart.py: the same): True = 129 .. 1,024 tokens on vlpet_amd.attention's forward-only long kernel
                          # wherever no dropout and no gradient is needed; the dense [B, H, L, L] mask is not built on that path
FUSE_QKV = True           # A/B switch: False = separate q / k / v projections in self-attention


LONG_ATTENTION_TRAIN = False   # switch (host/bart.py: the same): True = those lengths on the long TRAINING kernels wherever a call needs
                               # dropout or a gradient
FUSE_CROSS_KEYS = True    # A/B switch: False = every decoder block projects its own cross-attention keys (host/bart.py: the same fusion)


def _route(Lq, Lk, p, training, *tensors, grad=False):
    """attention.route under this module's switches (host/bart.py: the same)"""
    return A.route(Lq, Lk, p, training, A.needs_grad(*tensors, grad=grad), eager=EAGER_ATTENTION, long_on=LONG_ATTENTION,
                   long_train_on=LONG_ATTENTION_TRAIN)


def _long_applies(Lq, Lk, p, training, *tensors) -> bool:
    return _route(Lq, Lk, p, training, *tensors) == "long"


def _long_train_applies(Lq, Lk, p, training, *tensors) -> bool:
    return _route(Lq, Lk, p, training, *tensors) == "long_train"


class AttnSpec:
    """What a T5 attention adds to its scores, kept in parts: the relative-position bias shared by the batch ``rel``
    [1, H, Lq, Lk] (or None), the key padding ``keep`` [B, Lk] (1 = attend, or None) and causality.  ``dense()`` is the merged
    additive mask the reference builds (my_transformers/modeling_t5.py:640-660; src/modeling_t5.py:311-327 for the joint
    encoder) and torch's SDPA takes; ``fast()`` the form of vlpet_amd.attention's on-chip kernels -- an ``AttnBias`` built once per
    forward for all layers + the boolean key mask + the causal flag -- which removes the [B, H, L, L] mask tensor and the library's
    long-sequence flash kernels from the step (round 4: 220 -> ~70 us per encoder attention backward at B = 300, S = 56)."""

    def __init__(self, rel, keep, causal, rel_trainable=False):
        self.rel, self.keep, self.causal, self.rel_trainable = rel, keep, bool(causal), bool(rel_trainable)
        self._dense, self._fast = {}, None

    def dense(self, dtype):
        if dtype not in self._dense:
            m = None
            if self.rel is not None:
                m = self.rel
            if self.causal:
                L = self.rel.shape[-1]
                tri = torch.tril(torch.ones(L, L, device=self.rel.device))
                m = m + (1.0 - tri)[None, None] * -10000.0
            if self.keep is not None:
                pad = (1.0 - self.keep[:, None, None, :].to(torch.float32)) * (-10000.0 if self.rel is not None else -1e9)
                m = pad if m is None else m + pad
            self._dense[dtype] = None if m is None else m.to(dtype)
        return self._dense[dtype]

    def fast(self):
        """(AttnBias or None, key_mask uint8 or None) for the short-sequence kernels, or None when they do not apply."""
        if self.rel_trainable:
            return None
        if self._fast is None:
            # (the transposed copy is the short backward's: a forward-only long-kernel pass does not build it, nor does the long training
            # form, whose backward reads the table along keys; whoever needs it after all builds it on first use)
            lazy = (LONG_ATTENTION and not torch.is_grad_enabled()) or (
                LONG_ATTENTION_TRAIN and self.rel is not None and max(self.rel.shape[-2:]) > A.MAX_LEN)
            bias = A.AttnBias(self.rel, transposed=not lazy) if self.rel is not None else None
            km = None if self.keep is None else (self.keep > 0.5).to(torch.uint8).contiguous()
            self._fast = (bias, km)
        return self._fast


class T5Attention(nn.Module):
    """softmax(Q K^T + bias) V without the 1/sqrt(d) scale (folded into T5's initialisation); optional
    value-parallel adapter on the cross-attention value (``project_vpa``, :588-613)."""

    def __init__(self, config, is_decoder, has_relative_attention_bias=False, value_adapter=False):
        super().__init__()
        self.is_decoder = is_decoder
        self.n_heads, self.d_kv = config.num_heads, config.d_kv
        self.inner = self.n_heads * self.d_kv
        self.dropout = config.dropout_rate
        self.num_buckets = config.relative_attention_num_buckets
        d = config.d_model
        self.q = nn.Linear(d, self.inner, bias=False)
        self.k = nn.Linear(d, self.inner, bias=False)
        self.v = nn.Linear(d, self.inner, bias=False)
        self.o = nn.Linear(self.inner, d, bias=False)
        self.attn_value_parallel_adapter = None
        if value_adapter:
            self.attn_value_parallel_adapter = value_parallel_adapter(config)
        self.has_relative_attention_bias = has_relative_attention_bias
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(self.num_buckets, self.n_heads)

    def compute_bias(self, q_len, k_len):
        dev = self.relative_attention_bias.weight.device
        ctx = torch.arange(q_len, dtype=torch.long, device=dev)[:, None]
        mem = torch.arange(k_len, dtype=torch.long, device=dev)[None, :]
        bucket = relative_position_bucket(mem - ctx, bidirectional=not self.is_decoder, num_buckets=self.num_buckets)
        return self.relative_attention_bias(bucket).permute(2, 0, 1).unsqueeze(0)        # [1, H, q, k]

    def _shape(self, t, B):
        return t.view(B, -1, self.n_heads, self.d_kv).transpose(1, 2)

    def _fused_qkv(self, dtype):
        """The frozen q | k | v projections of a self-attention as one [3 inner, d] weight (common.derived_weights; T5 has no biases)"""
        return derived_weights(self, "_qkv_cache", (self.q, self.k, self.v), dtype)[0]

    def forward(self, hidden, bias, kv=None, task=None, k_pre=None):
        """``k_pre`` = (k, k_slot): this block's cross-attention keys, a column block of the decoder's fused key projection (T5Decoder._cross_keys)"""
        B, Lq, _ = hidden.shape
        src = hidden if kv is None else kv
        k_slot = None
        spec = bias if isinstance(bias, AttnSpec) else None
        kind = _route(Lq, Lq, self.dropout, self.training, hidden) if kv is None and FUSE_QKV and spec is not None else None
        if (kind is not None and hidden.is_cuda and hidden.dtype == torch.bfloat16 and self.d_kv == A.HEAD_DIM
                and not any(m.weight.requires_grad for m in (self.q, self.k, self.v))):
            fast = spec.fast()
            if fast is not None:
                # self-attention with frozen projections: ONE [d -> 3 inner] GEMM each way (T5's projections carry no bias), the
                # attention kernels read / write the q | k | v column blocks in place -- 2 library launches instead of 6 and one
                # input gradient instead of three (at the per-rank batch of an 8-GPU run each of those GEMMs is a ~9 us launch)
                w = self._fused_qkv(hidden.dtype)
                if FUSE_RESIDUAL_GRAD and FUSE_NORM_GRAD and torch.is_grad_enabled() and hidden.requires_grad:
                    qkv = VF.linear_acc(hidden, None, (w, None))
                else:
                    qkv = F.linear(hidden, w)
                out = A.attend_qkv(kind, qkv, self.n_heads, fast[1], spec.causal, self.dropout, self.training, scale=1.0, bias=fast[0])
                return _linear(self.o, out)
        fused = (FUSE_RESIDUAL_GRAD and FUSE_NORM_GRAD and hidden.is_cuda and torch.is_grad_enabled() and src.requires_grad
                 and not any(m.weight.requires_grad for m in (self.q, self.k, self.v)))
        if fused:
            # the projections that read one tensor are ONE autograd node whose dgrad GEMMs accumulate into one gradient
            # (functional.linear_acc): q | k | v of a self-attention; k | v of a cross-attention, onto K2's parked d/dsrc
            if kv is None:
                q, k, v = VF.linear_acc(hidden, None, self.q, self.k, self.v)
            else:
                q = _linear(self.q, hidden)
                kv_link = VF.ResidualLink() if self.attn_value_parallel_adapter is not None else None
                if k_pre is not None:
                    (k, k_slot), v = k_pre, VF.linear_acc(src, kv_link, self.v)
                else:
                    k, v = VF.linear_acc(src, kv_link, self.k, self.v)
                if self.attn_value_parallel_adapter is not None:
                    v = self.attn_value_parallel_adapter(src, task, y=v, link=kv_link)    # K2
        else:
            q, k, v = _linear(self.q, hidden), _linear(self.k, src), _linear(self.v, src)
            if kv is not None and self.attn_value_parallel_adapter is not None:
                v = self.attn_value_parallel_adapter(src, task, y=v)                      # K2
        kind = _route(Lq, k.shape[1], self.dropout, self.training, q, k, v) if spec is not None and self.d_kv == A.HEAD_DIM else None
        if A.fits(kind, q, k, v, self.n_heads):
            fast = spec.fast()
            if fast is not None:        # on-chip kernels: bias shared by the batch + boolean key mask + causal flag; T5 has no 1/sqrt(d)
                out = A.attend(kind, q, k, v, self.n_heads, fast[1], spec.causal, self.dropout, self.training, scale=1.0, bias=fast[0],
                               k_slot=k_slot)
                return _linear(self.o, out)
        mask = spec.dense(q.dtype) if spec is not None else (None if bias is None else bias.to(q.dtype))
        out = F.scaled_dot_product_attention(self._shape(q, B), self._shape(k.contiguous(), B), self._shape(v, B), attn_mask=mask,
                                             dropout_p=self.dropout if self.training else 0.0, scale=1.0)
        return _linear(self.o, out.transpose(1, 2).reshape(B, Lq, self.inner))


    # ---- generate(): one decoder token against the caches (decode.decode_attention, scale 1: T5 has no 1/sqrt(d))
    def step_self(self, n, k_cache, v_cache, pos, bias_row, key_rows=None, pos_dev=None):
        """causal self-attention of the normed token n [B, 1, d] at ``pos``; ``bias_row`` [H, >= pos + 1]: row ``pos`` of the
        decoder's relative position bias.  ``pos_dev``: the position word instead of ``pos``; ``bias_row`` is then the whole bias
        table and ``key_rows`` both ping-pong halves (decode.decode_attention)"""
        E = self.inner
        if FUSE_QKV:
            qkv = F.linear(n[:, 0], self._fused_qkv(n.dtype))
            q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        else:
            q, k, v = _linear(self.q, n)[:, 0], _linear(self.k, n)[:, 0], _linear(self.v, n)[:, 0]
        out = D.decode_attention(q, k_cache, v_cache, self.n_heads, pos=pos, k_new=k, v_new=v, bias=bias_row, scale=1.0,
                                 key_rows=key_rows, pos_dev=pos_dev)
        return _linear(self.o, out[:, None])

    def cross_values(self, enc, task=None):
        """the cross-attention value cache with the value-parallel adapter (K2) applied once (``project_vpa`` on the cached value)"""
        v = _linear(self.v, enc)
        if self.attn_value_parallel_adapter is not None:
            v = self.attn_value_parallel_adapter(enc, task, y=v)
        return v

    def step_cross(self, n, k_cache, v_cache, key_mask, group=1):
        out = D.decode_attention(_linear(self.q, n)[:, 0], k_cache, v_cache, self.n_heads, key_mask=key_mask, scale=1.0, group=group)
        return _linear(self.o, out[:, None])


class T5DenseReluDense(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.wi = nn.Linear(config.d_model, config.d_ff, bias=False)
        self.wo = nn.Linear(config.d_ff, config.d_model, bias=False)
        self.dropout = config.dropout_rate

    def forward(self, x):
        h = ffn_activation(_linear(self.wi, x), "relu", self.dropout, self.training)
        return _linear(self.wo, h)


def _generated(sub, block_adapters, block):
    """the generated adapter of sublayer module ``sub`` for its ``block`` type, None where it has none (no Hyperformer, or the
    cross-attention without add_adapter_cross_attn)"""
    return None if sub.adapter_hypernet is None else block_adapters[block]


class T5LayerSelfAttention(nn.Module):
    def __init__(self, config, is_decoder, has_relative_attention_bias):
        super().__init__()
        self.config, self.is_decoder, self.p = config, is_decoder, config.dropout_rate
        self.SelfAttention = T5Attention(config, is_decoder, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        if not is_decoder:
            build_pet(self, config, config.d_model, ("attn",))
        # my_transformers/modeling_t5.py:701-702, 744-745
        self.attn_adapter = AdapterController(config.adapter_config) if sequential_adapters(config, "decoder" if is_decoder else "encoder") else None
        self.adapter_hypernet = MetaLayersAdapterController(config.adapter_config) if hyperformer(config) else None      # (:749-751)

    def forward(self, hidden, bias, task=None, block_adapters=None):
        nl = _new_norm_link(hidden)
        y = self.SelfAttention(_normed(self.layer_norm, hidden, nl), bias)
        if not self.is_decoder and has_pet(self, "attn"):                                 # K1 (x1 = un-normalised stream) + K5
            return _pet_then_tail(self, "attn", hidden, y, None, self.p, self.training, self.config, norm_link=nl)
        return _tail_or_adapter(self.attn_adapter, task, hidden, y, self.p, self.training, nl, self, _generated(self, block_adapters, "self_attention"))


class T5LayerCrossAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.p = config.dropout_rate
        self.EncDecAttention = T5Attention(config, True, False,
                                           value_adapter=bool(config.use_decoder_enc_attn_value_parallel_adapter_down_dim))
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        # my_transformers/modeling_t5.py:847-850
        self.enc_attn_adapter = (AdapterController(config.adapter_config)
                                 if sequential_adapters(config, "decoder") and config.add_adapter_cross_attn else None)
        self.adapter_hypernet = (MetaLayersAdapterController(config.adapter_config)
                                 if hyperformer(config) and config.add_adapter_cross_attn else None)                    # (:852-854)

    def forward(self, hidden, enc, bias, task=None, k_pre=None, block_adapters=None):
        nl = _new_norm_link(hidden)
        y = self.EncDecAttention(_normed(self.layer_norm, hidden, nl), bias, kv=enc, task=task, k_pre=k_pre)
        return _tail_or_adapter(self.enc_attn_adapter, task, hidden, y, self.p, self.training, nl, self, _generated(self, block_adapters, "cross_attention"))


class T5LayerFF(nn.Module):
    def __init__(self, config, is_decoder):
        super().__init__()
        self.config, self.is_decoder, self.p = config, is_decoder, config.dropout_rate
        self.DenseReluDense = T5DenseReluDense(config)
        self.layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        if not is_decoder:
            build_pet(self, config, config.d_model, ("ff",))
        # my_transformers/modeling_t5.py:307-308, 350-351
        self.ff_adapter = AdapterController(config.adapter_config) if sequential_adapters(config, "decoder" if is_decoder else "encoder") else None
        self.adapter_hypernet = MetaLayersAdapterController(config.adapter_config) if hyperformer(config) else None      # (:355-357)

    def forward(self, hidden, task=None, block_adapters=None):
        nl = _new_norm_link(hidden)
        y = self.DenseReluDense(_normed(self.layer_norm, hidden, nl))
        if not self.is_decoder and has_pet(self, "ff"):
            return _pet_then_tail(self, "ff", hidden, y, None, self.p, self.training, self.config, norm_link=nl)      # K1 + K5
        return _tail_or_adapter(self.ff_adapter, task, hidden, y, self.p, self.training, nl, self, _generated(self, block_adapters, "feed_forward"))


class T5Block(nn.Module):
    def __init__(self, config, is_decoder, has_relative_attention_bias):
        super().__init__()
        self.is_decoder = is_decoder
        layers = [T5LayerSelfAttention(config, is_decoder, has_relative_attention_bias)]
        if is_decoder:
            layers.append(T5LayerCrossAttention(config))
        layers.append(T5LayerFF(config, is_decoder))
        self.layer = nn.ModuleList(layers)

    def forward(self, hidden, self_bias, enc=None, cross_bias=None, task=None, k_pre=None, block_adapters=None):
        hidden = self.layer[0](hidden, self_bias, task, block_adapters)
        if self.is_decoder:
            hidden = self.layer[1](hidden, enc, cross_bias, task, k_pre=k_pre, block_adapters=block_adapters)
        return self.layer[-1](hidden, task, block_adapters)


def _block_step(blk, x, cache, pos, state, bias_row, task=None, block_adapters=None):
    """generate(): one decoder block on the token x [B, 1, d]; ``cache`` = this block's (self k, self v, cross k, cross v) of ``state``
    (decode.DecodeState), ``bias_row`` = row ``pos`` of its bias table.  The tails are forward's (_tail_linked: on the GPU each fused
    with the next sublayer's norm)."""
    sa, ca, ff = blk.layer[0], blk.layer[1], blk.layer[-1]
    ks, vs, kx, vx = cache
    kr, pd = state.key_rows, state.pos_dev
    y = sa.SelfAttention.step_self(sa.layer_norm(x), ks, vs, pos, bias_row,
                                   key_rows=kr if kr is None or pd is not None else kr[pos & 1], pos_dev=pd)
    x = _tail_or_adapter(sa.attn_adapter, task, x, y, sa.p, sa.training, None, sa, _generated(sa, block_adapters, "self_attention"))
    y = ca.EncDecAttention.step_cross(ca.layer_norm(x), kx, vx, state.key_mask, group=state.group)
    x = _tail_or_adapter(ca.enc_attn_adapter, task, x, y, ca.p, ca.training, None, ca, _generated(ca, block_adapters, "cross_attention"))
    y = ff.DenseReluDense(ff.layer_norm(x))
    return _tail_or_adapter(ff.ff_adapter, task, x, y, ff.p, ff.training, None, ff, _generated(ff, block_adapters, "feed_forward"))


def _pad_bias(mask, dtype):
    """[B, K] keep-mask -> additive [B, 1, 1, K] (the reference's (1 - mask) * -10000 form)."""
    return (1.0 - mask[:, None, None, :].to(torch.float32)) * -10000.0


def _install_hyper_net(stack, config, task_embed, num_layers, is_decoder):
    """my_transformers/modeling_t5.py:1097-1106: the shared TaskEmbeddingController under the stack's own name too, and the stack's
    hyper-network (with the cross-attention generators in the decoder), registered right behind ``embed_tokens`` as there; without the
    flag no attribute and no state-dict key"""
    if hyperformer(config):
        stack.task_embed = task_embed
        stack.adapter_layers_hyper_net = new_hyper_net(config, num_layers, is_decoder)


def _stack_block_adapters(stack, task, x):
    """every block's generated adapters for ``task`` (one generator launch), or a list of None without Hyperformer"""
    if getattr(stack, "adapter_layers_hyper_net", None) is None:
        return [None] * len(stack.block)
    return block_adapters(stack.adapter_layers_hyper_net, stack.task_embed, task, x)


class JointEncoder(nn.Module):
    def __init__(self, config, embed_tokens, task_embed=None):
        super().__init__()
        self.config = config
        self.embed_tokens = embed_tokens
        _install_hyper_net(self, config, task_embed, config.num_layers, False)
        self.block = nn.ModuleList([T5Block(config, False, i == 0) for i in range(config.num_layers)])
        self.final_layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        _wire_next_norms(self.block, self.final_layer_norm)
        self.p = config.dropout_rate
        vcfg = copy.copy(config)
        self.visual_embedding = VisualEmbedding(vcfg, embed_tokens, rms_norm=True)
        self.downsample = None
        if config.downsample:
            s = int(config.n_boxes ** 0.5)
            self.downsample = Downsample((s, s))
        # src/modeling_t5.py:198-201 (prompt tuning); without the flag no attribute and no state-dict key, as before
        if getattr(config, "encoder_prompt_config", None) is not None:
            self.prompt_modules = PromptController(config.encoder_prompt_config)

    def forward(self, input_ids, vis_inputs, attention_mask=None, task=None):
        B, L = input_ids.shape
        x = self.embed_tokens(input_ids)
        vis = self.visual_embedding(*unpack_vis_inputs(vis_inputs, self.downsample, x.dtype)).to(x.dtype)             # K4
        V = vis.shape[1]
        if attention_mask is None:
            attention_mask = input_ids.ne(self.config.pad_token_id)
        keep = attention_mask.to(torch.float32)
        if getattr(self, "prompt_modules", None) is not None:
            # src/modeling_t5.py:236-238, 271-276: [prompt | text | visual]; the prompt rows count as text for the relative-position
            # bias (L = P + text length) and are always attended.  The MLP runs on the P rows once, not on B * P.
            from ..act import prefix_concat_dropout
            pre = self.prompt_modules.prompt_rows(task).to(x.dtype)
            x = prefix_concat_dropout(pre, x, vis, self.p, self.training)
            keep = torch.cat([torch.ones(B, pre.shape[0], device=x.device), keep], dim=1)
            L += pre.shape[0]
        else:
            from ..act import concat_dropout
            x = concat_dropout(x, vis, self.p, self.training)      # cat + dropout (src/modeling_t5.py:263, 300): one pass each way
        full = torch.cat([keep, torch.ones(B, V, device=x.device)], dim=1)
        # relative position bias only between text positions (src/modeling_t5.py:311-327)
        sa0 = self.block[0].layer[0].SelfAttention
        text_bias = sa0.compute_bias(L, L)
        rel = text_bias.new_zeros(1, text_bias.shape[1], L + V, L + V)
        rel[:, :, :L, :L] = text_bias
        bias = AttnSpec(rel, full, causal=False, rel_trainable=sa0.relative_attention_bias.weight.requires_grad and torch.is_grad_enabled())
        for blk, ba in zip(self.block, _stack_block_adapters(self, task, x)):
            x = blk(x, bias, task=task, block_adapters=ba)
        x = F.dropout(self.final_layer_norm(x), p=self.p, training=self.training)
        return x, full


class T5Decoder(nn.Module):
    def __init__(self, config, embed_tokens, task_embed=None):
        super().__init__()
        self.config = config
        self.embed_tokens = embed_tokens
        _install_hyper_net(self, config, task_embed, config.num_decoder_layers, True)
        self.block = nn.ModuleList([T5Block(config, True, i == 0) for i in range(config.num_decoder_layers)])
        self.final_layer_norm = T5LayerNorm(config.d_model, eps=config.layer_norm_epsilon)
        _wire_next_norms(self.block, self.final_layer_norm)
        self.p = config.dropout_rate

    def _cross_keys_ok(self, enc, cross_bias) -> bool:
        """The blocks' cross-attention key projections as ONE GEMM (functional.cross_key_blocks; host/bart.py BartDecoder._cross_keys_ok)"""
        if not FUSE_CROSS_KEYS or EAGER_ATTENTION or len(self.block) < 2 or not enc.is_cuda or enc.dtype != torch.bfloat16:
            return False
        if not (FUSE_RESIDUAL_GRAD and FUSE_NORM_GRAD and torch.is_grad_enabled() and enc.requires_grad):
            return False
        atts = [blk.layer[1].EncDecAttention for blk in self.block]
        # (past the short kernels' length the long training kernels read a block in place and write dk into the shared slot; a gradient is
        # needed here: see above)
        if _route(enc.shape[1], enc.shape[1], atts[0].dropout, self.training, grad=True) is None or atts[0].d_kv != A.HEAD_DIM or cross_bias.fast() is None:
            return False
        return not any(m.weight.requires_grad or m.bias is not None for a in atts for m in (a.q, a.k, a.v))

    def _cross_keys(self, enc):
        w, _ = derived_weights(self, "_ck_cache", [blk.layer[1].EncDecAttention.k for blk in self.block], enc.dtype)
        return VF.cross_key_blocks(enc, w, None, len(self.block))

    def forward(self, input_ids, enc, enc_keep, task=None):
        B, L = input_ids.shape
        x = F.dropout(self.embed_tokens(input_ids), p=self.p, training=self.training)
        sa0 = self.block[0].layer[0].SelfAttention
        self_bias = AttnSpec(sa0.compute_bias(L, L), None, causal=True,
                             rel_trainable=sa0.relative_attention_bias.weight.requires_grad and torch.is_grad_enabled())
        cross_bias = AttnSpec(None, enc_keep, causal=False)      # (dense form: invert_attention_mask, (1 - keep) * -1e9 in fp32)
        n = len(self.block)
        fused_keys = self._cross_keys_ok(enc, cross_bias)
        encs = VF.fanout(enc, n + (1 if fused_keys else 0))         # one gradient sum for the encoder output instead of autograd's pairwise adds
        ks = self._cross_keys(encs[n]) if fused_keys else None
        bas = _stack_block_adapters(self, task, x)
        for i, (blk, e) in enumerate(zip(self.block, encs)):
            x = blk(x, self_bias, e, cross_bias, task, k_pre=None if ks is None else (ks[0][i], None if ks[1] is None else (ks[1], i)),
                    block_adapters=bas[i])
        return F.dropout(self.final_layer_norm(x), p=self.p, training=self.training)


    def init_cache(self, enc, key_mask, task, max_length, num_beams=1):
        """generate(): the decode.DecodeState of a call over ``enc`` (as host/bart.py BartDecoder.init_cache: the cross-attention keys
        as column blocks of ONE fused projection on the GPU), with the relative position bias of every query position as its
        [max_length, H, max_length] fp32 table (row ``pos`` = compute_bias(max_length, max_length)[0, :, pos])."""
        atts = [blk.layer[1].EncDecAttention for blk in self.block]
        if FUSE_CROSS_KEYS and not EAGER_ATTENTION and len(atts) >= 2 and enc.is_cuda:
            ks = self._cross_keys(enc)[0]
        else:
            ks = [_linear(a.k, enc) for a in atts]
        vs = [a.cross_values(enc, task) for a in atts]
        sa0 = self.block[0].layer[0].SelfAttention
        table = sa0.compute_bias(max_length, max_length)[0].permute(1, 0, 2).float().contiguous()        # [H, q, k] -> [q, H, k]
        return D.new_decode_state(enc, sa0.inner, max_length, ks, vs, key_mask, num_beams, bias_table=table)

    def block_adapters(self, task, x):
        """generate(): every block's generated adapters for ``task``, once per call (host/bart.py BartDecoder.block_adapters)"""
        return _stack_block_adapters(self, task, x)

    def step(self, tok, pos, state, task=None, block_adapters=None):
        x = F.dropout(self.embed_tokens(tok)[:, None], p=self.p, training=self.training)
        bias_row = state.bias_table if state.pos_dev is not None else state.bias_table[pos]    # (the kernel takes row *pos_dev)
        bas = block_adapters if block_adapters is not None else [None] * len(self.block)
        for blk, c, ba in zip(self.block, state.layers, bas):
            x = _block_step(blk, x, c, pos, state, bias_row, task, ba)
        return F.dropout(self.final_layer_norm(x), p=self.p, training=self.training)[:, 0]


class VLT5(nn.Module):
    """``forward`` returns (per-token loss [B, L], logits) like the reference's ``reduce_loss=False`` path
    (src/modeling_t5.py:670-700); the LM head is the shared embedding, inputs rescaled by d_model**-0.5."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.shared = nn.Embedding(config.vocab_size, config.d_model)
        # my_transformers/modeling_t5.py:1651-1666: ONE TaskEmbeddingController, registered here and under both stacks
        task_embed = None           # (without the flag no attribute at all: the module tree of every other flag set is unchanged)
        if hyperformer(config):
            self.shared_task_embed = task_embed = TaskEmbeddingController(config.adapter_config)
        self.encoder = JointEncoder(config, self.shared, task_embed)
        self.decoder = T5Decoder(config, self.shared, task_embed)
        install_shared_phm_rule(self, [self.encoder, self.decoder], config.adapter_config)        # (Compacter with shared_phm_rule)
        self.apply(self._init_weights)
        self.register_load_state_dict_post_hook(lambda module, incompatible: VF.invalidate_caches())   # (see host/bart.py)

    def _init_weights(self, m):
        # my_transformers/modeling_t5.py:1026-1066: T5's Mesh-TensorFlow rules for its own layers; adapter / gate
        # Linears keep the nn.Linear default (no generic branch there)
        f = self.config.initializer_factor
        d, dkv, H = self.config.d_model, self.config.d_kv, self.config.num_heads
        if isinstance(m, T5LayerNorm):
            m.weight.data.fill_(f * 1.0)
        elif isinstance(m, VLT5):
            m.shared.weight.data.normal_(0.0, f * 1.0)
        elif isinstance(m, T5DenseReluDense):
            m.wi.weight.data.normal_(0.0, f * d ** -0.5)
            m.wo.weight.data.normal_(0.0, f * self.config.d_ff ** -0.5)
        elif isinstance(m, T5Attention):
            m.q.weight.data.normal_(0.0, f * (d * dkv) ** -0.5)
            m.k.weight.data.normal_(0.0, f * d ** -0.5)
            m.v.weight.data.normal_(0.0, f * d ** -0.5)
            m.o.weight.data.normal_(0.0, f * (H * dkv) ** -0.5)
            if m.has_relative_attention_bias:
                m.relative_attention_bias.weight.data.normal_(0.0, f * d ** -0.5)

    def forward(self, input_ids, vis_inputs, labels, task, attention_mask=None, no_padding=False):
        cfg = self.config       # (no_padding: accepted for interface symmetry with host/bart.py; the T5 bias always carries the mask)
        enc, keep = self.encoder(input_ids, vis_inputs, attention_mask, task)
        dec_in = shift_right(labels, cfg.pad_token_id, cfg.decoder_start_token_id)
        h = self.decoder(dec_in, enc, keep, task) * (cfg.d_model ** -0.5)
        return lm_loss(h, self.shared.weight, labels)

    def generate(self, input_ids, vis_inputs, task, attention_mask=None, max_length=20, min_length=0, no_repeat_ngram_size=0,
                 eos_token_id=None, pad_token_id=None, no_padding=False, num_beams=1, length_penalty=1.0, early_stopping=False,
                 graph=False):
        """Greedy search with HF 4.2.1 semantics on per-block key / value caches (see host/bart.py VLBart.generate).  eos / pad
        default to T5's 1 / 0; the output starts with decoder_start_token_id (0).  ``num_beams`` > 1: HF 4.2.1 beam search as in
        VLBart.generate (T5 forces no eos).  ``graph=True``: the captured, replayed decode step, as there."""
        from ..lmloss import _padded_head
        cfg = self.config
        eos = getattr(cfg, "eos_token_id", 1) if eos_token_id is None else eos_token_id
        pad = cfg.pad_token_id if pad_token_id is None else pad_token_id
        with eval_no_grad(self):
            enc, keep = self.encoder(input_ids, vis_inputs, attention_mask, task)
            state = self.decoder.init_cache(enc, (keep > 0.5).contiguous(), task, max_length, num_beams=int(num_beams))
            bas = self.decoder.block_adapters(task, enc)
            V = self.shared.weight.shape[0]
            head = _padded_head(self.shared.weight, enc.dtype)
            scale = cfg.d_model ** -0.5

            def make_step(st):
                return lambda tok, pos: F.linear(self.decoder.step(tok, pos, st, task, bas) * scale, head)
            if graph:
                gs = D.GenSettings(cfg.decoder_start_token_id, eos, int(pad), int(max_length), int(min_length),
                                   int(no_repeat_ngram_size), int(num_beams), float(length_penalty), bool(early_stopping), False)
                return D.graph_generate(self, state, make_step, V, cfg.num_heads, head, gs, key_extra=(task,))[0]
            return D.generate(make_step(state), V, enc.shape[0], enc.device, state.key_rows, cfg.decoder_start_token_id, eos, pad,
                              max_length, min_length, no_repeat_ngram_size, int(num_beams), length_penalty, early_stopping,
                              force_eos=False)
