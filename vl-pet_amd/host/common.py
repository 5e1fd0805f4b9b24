"""What the two host models (host/bart.py, host/t5.py) share, written once.  No A/B switches and no swappable hooks live here: the
harnesses set those as attributes of ``host.bart`` / ``host.t5``, and a helper that depends on one takes it as an argument."""
from __future__ import annotations

import contextlib
import copy

import torch

from .. import functional as VF
from ..adapters import AdapterController


def derived_weights(owner, slot, mods, dtype):
    """``(cat of the modules' weights [sum out, in], cat of their biases or None)`` in ``dtype``: the fused q | k | v projection of a
    self-attention, the fused cross-attention key projection of a decoder.  A derived cache kept as the plain attribute ``slot`` of
    ``owner`` -- never a parameter or buffer: the state dict keeps the separate modules -- and rebuilt when one of the tensors
    changes (data pointer, version), after a cast of the frozen weights or a checkpoint load (functional.FROZEN_EPOCH)."""
    key = tuple((m.weight.data_ptr(), m.weight._version) if m.bias is None else
                (m.weight.data_ptr(), m.weight._version, m.bias.data_ptr(), m.bias._version) for m in mods) + (dtype, VF.FROZEN_EPOCH)
    c = getattr(owner, slot, None)
    if c is None or c[0] != key:
        with torch.no_grad():
            w = torch.cat([m.weight.to(dtype) for m in mods], 0).contiguous()
            b = None if mods[0].bias is None else torch.cat([m.bias.to(dtype) for m in mods], 0).contiguous()
        c = (key, w, b)
        setattr(owner, slot, c)
    return c[1], c[2]


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
