"""Output tensors for the streaming-kernel tests: the body is pre-filled with NaN (an element the kernel never writes fails any
comparison), and behind it lie extra trailing rows / elements filled with a sentinel byte pattern that must come back untouched
(a write past the end of the output -- a wrong stride, a piece guard off by one -- lands there).  Plain tensors, no allocator tricks."""
import torch

PAD_ROWS = 4            # extra trailing rows of a [rows, d] output
PAD_FLAT = 64           # extra trailing elements of a flat output
SENTINEL = 0x5A         # every pad byte (bf16 0x5A5A and fp32 0x5A5A5A5A are finite numbers, not NaN: a copy keeps the bits)


def padded_rows(rows: int, d: int, dtype, device="cuda"):
    """-> (buf [rows + PAD_ROWS, d], body = buf[:rows]): body NaN (0xFF bytes for uint8), pad = sentinel bytes."""
    buf = torch.empty(rows + PAD_ROWS, d, dtype=dtype, device=device)
    buf.view(torch.uint8)[rows:] = SENTINEL
    buf[:rows] = 0xFF if dtype == torch.uint8 else float("nan")
    return buf, buf[:rows]


def padded_flat(n: int, dtype, device="cuda"):
    """-> (buf [n + PAD_FLAT], body = buf[:n])"""
    buf = torch.empty(n + PAD_FLAT, dtype=dtype, device=device)
    buf.view(torch.uint8)[n * buf.element_size():] = SENTINEL
    buf[:n] = 0xFF if dtype == torch.uint8 else float("nan")
    return buf, buf[:n]


def pad_intact(buf: torch.Tensor, body: torch.Tensor) -> bool:
    """True iff every byte behind ``body`` inside ``buf`` still holds the sentinel."""
    nbytes = body.numel() * body.element_size()
    return bool((buf.reshape(-1).view(torch.uint8)[nbytes:] == SENTINEL).all())
