"""The two objects the autograd functions move gradients with (functional.ResidualLink, functional.GradSlot), on CPU tensors:
no kernel runs here, only the protocol every backward relies on."""
import pytest
import torch

import vlpet_amd.functional as VF


# ---- ResidualLink ---------------------------------------------------------------------------------------------------------
def test_link_arm_and_if_armed():
    link = VF.ResidualLink()
    assert not link.armed and not link.holds
    assert VF.ResidualLink.if_armed(None) is None
    assert VF.ResidualLink.if_armed(link) is None
    assert link.arm() is link and link.armed
    assert VF.ResidualLink.if_armed(link) is link


def test_link_take_on_an_empty_link():
    link = VF.ResidualLink().arm()
    assert link.take((3, 4), torch.float32) is None
    assert link.take((3, 4), torch.float32, writable=True) is None
    assert link.armed and not link.holds


def test_link_take_returns_the_parked_storage_when_it_fits():
    link = VF.ResidualLink().arm()
    g = torch.randn(6, 8)
    link.park(g)
    assert link.holds
    t = link.take((6, 8), torch.float32)
    assert t.data_ptr() == g.data_ptr() and t.shape == (6, 8) and not link.holds
    assert link.take((6, 8), torch.float32) is None          # taken once


@pytest.mark.parametrize("writable", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_link_take_repairs_shape_dtype_and_layout(shared, writable):
    B, L, d = 2, 3, 8
    cases = [
        (torch.randn(B, L, d), (B * L, d), torch.float32),                                    # [B, L, d] taken as [B * L, d]
        (torch.randn(B * L, d).bfloat16(), (B * L, d), torch.float32),                        # bf16 taken as fp32
        (torch.randn(d, B * L).t(), (B * L, d), torch.float32),                               # not contiguous
        (torch.randn(d, L, B).bfloat16().permute(2, 1, 0), (B * L, d), torch.float32),        # all three at once
    ]
    for g, shape, dtype in cases:
        keep = g.clone()
        link = VF.ResidualLink().arm()
        link.park(g, shared=shared)
        t = link.take(shape, dtype, writable=writable)
        assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and not link.holds
        assert torch.equal(t, keep.reshape(shape).to(dtype))
        if writable and shared:
            t.add_(1.0)
            assert torch.equal(g, keep)             # whatever repair ran, the parked tensor is nobody's accumulator


def test_link_shared_and_writable_decide_aliasing():
    g = torch.randn(5, 4)
    keep = g.clone()
    link = VF.ResidualLink().arm()
    link.park(g, shared=True)
    t = link.take((5, 4), torch.float32, writable=True)
    assert t.data_ptr() != g.data_ptr() and torch.equal(t, g)
    t.add_(1.0)
    assert torch.equal(g, keep)                     # the in-place add did not reach the parked tensor
    link.park(g, shared=True)
    assert link.take((5, 4), torch.float32).data_ptr() == g.data_ptr()                       # read only: the alias
    link.park(g)
    assert link.take((5, 4), torch.float32, writable=True).data_ptr() == g.data_ptr()        # unshared: the caller may write into it
    link.park(g.view(20), shared=True)
    t = link.take((5, 4), torch.float32, writable=True)                                      # a reshaped view is still the shared storage
    assert t.data_ptr() != g.data_ptr() and torch.equal(t, g)


def test_link_second_park_raises_and_take_clears_the_shared_flag():
    g, h = torch.randn(3, 4), torch.randn(3, 4)
    link = VF.ResidualLink().arm()
    link.park(g, shared=True)
    with pytest.raises(RuntimeError):
        link.park(h)
    assert link.take((3, 4), torch.float32).data_ptr() == g.data_ptr()       # the first one is still there
    assert not link.holds
    link.park(h)                                    # a plain park after a shared one: unshared
    assert link.take((3, 4), torch.float32, writable=True).data_ptr() == h.data_ptr()


# ---- GradSlot -------------------------------------------------------------------------------------------------------------
class FakeSink:
    """What functional.grad_slot needs of train.GradSink: ``view``, ``take()`` (the view, or None at a second use), ``done()``."""

    def __init__(self, view, offers=True):
        self.view, self.offers, self.takes, self.dones = view, offers, 0, 0

    def take(self):
        self.takes += 1
        return self.view if self.offers else None

    def done(self):
        self.dones += 1


def _param(shape, dtype=torch.float32, sink=None, block=False):
    p = torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))
    if sink is not None:
        setattr(p, "_vlpet_block_sink" if block else "_vlpet_sink", sink)
    return p


def test_slot_with_a_matching_sink_writes_into_its_view():
    sink = FakeSink(torch.zeros(4, 6))
    p = _param((4, 6), sink=sink)
    s = VF.grad_slot(p, (4, 6))
    assert s.t is sink.view and s.ptr == sink.view.data_ptr() and s.sunk and sink.takes == 1 and sink.dones == 0
    assert s.finish() is None and sink.dones == 1
    assert not VF.grad_slot(p, (4, 6), block=True).sunk and sink.takes == 1        # the block sink is another attribute


def test_slot_ignores_a_sink_of_another_shape_or_device():
    for view in (torch.zeros(6, 4), torch.zeros(4, 6, device="meta")):
        sink = FakeSink(view)
        p = _param((4, 6), sink=sink)
        s = VF.grad_slot(p, (4, 6))
        assert not s.sunk and sink.takes == 0
        assert s.t.shape == (4, 6) and s.t.dtype == torch.float32 and s.t.device == p.device
        s.t.fill_(2.0)
        assert s.finish() is s.t and sink.dones == 0


def test_slot_falls_back_when_the_sink_was_already_taken():
    sink = FakeSink(torch.zeros(8), offers=False)
    p = _param((8,), sink=sink)
    s = VF.grad_slot(p, (8,))
    assert sink.takes == 1 and not s.sunk and s.t is not sink.view and s.t.dtype == torch.float32
    assert s.finish() is s.t and sink.dones == 0


def test_slot_returns_the_parameters_dtype():
    p = _param((3, 5), dtype=torch.bfloat16)
    s = VF.grad_slot(p, (3, 5))
    assert s.t.dtype == torch.float32 and not s.sunk
    s.t.copy_(torch.randn(3, 5))
    g = s.finish()
    assert g.dtype == torch.bfloat16 and torch.equal(g, s.t.to(torch.bfloat16))


def test_slot_finish_heads():
    n_heads, rh, d = 3, 2, 4
    heads = [_param((rh, d), dtype=torch.bfloat16) for _ in range(n_heads)]
    s = VF.grad_slot(heads[0], (n_heads * rh, d), block=True)
    s.t.copy_(torch.arange(n_heads * rh * d, dtype=torch.float32).view(n_heads * rh, d))
    gs = s.finish_heads(heads)
    assert len(gs) == n_heads
    for i, g in enumerate(gs):
        assert g.dtype == torch.bfloat16 and torch.equal(g, s.t[i * rh:(i + 1) * rh].to(torch.bfloat16))
    sink = FakeSink(torch.zeros(n_heads * rh, d))
    heads[0]._vlpet_block_sink = sink
    s = VF.grad_slot(heads[0], (n_heads * rh, d), block=True)
    assert s.sunk and s.t is sink.view
    assert s.finish_heads(heads) == [None] * n_heads and sink.dones == 1


def test_scratch_slot_returns_nothing():
    s = VF.GradSlot.scratch((7,), torch.device("cpu"))
    assert s.t.shape == (7,) and s.t.dtype == torch.float32 and not s.sunk
    assert s.finish() is None
