"""Guard-band buffers for the memory-contract tests (tests/test_gpu_memory_contract.py; a plain helper module like _tiny_llama.py).

``Guarded(nbytes, guard_bytes, body_fill, guard_fill, device)`` is ONE uint8 allocation laid out as ``[low guard | body | high guard]``:

* the body starts on a 256-byte boundary and the high guard begins at byte ``nbytes`` of the body exactly (no rounding: a 2-byte overrun is seen);
* ``.ptr`` is the body pointer, ``.view(dtype, shape)`` a typed view of the body;
* ``.assert_intact(name)`` compares both guards with their fill on the device (one sync per call) and, on damage, reports the side, the first and the last
  damaged byte offset RELATIVE TO THE BODY (negative: below it; >= nbytes: behind it) and the count of damaged bytes -- the evidence a fix starts from.

Fills: guards of outputs and workspaces 0xA5; guards of inputs 0xFF (NaN as fp16 / bf16 / fp32, -1 as int64); output bodies 0xFF (an unwritten element is
a NaN); workspace bodies 0x00 (the header contract of include/gptq_mi355x.h).  The guards are sized by the caller so that a whole stray tile still lands in
memory the test owns: ``guard_for(row_bytes)`` = max(64 KiB, 128 rows), a workspace max(64 KiB, its own size)."""
import torch

OUT_GUARD = 0xA5      # outputs and workspaces
IN_GUARD = 0xFF       # inputs: NaN in every float format, -1 as int64
ALIGN = 256


def guard_for(row_bytes: int = 0, rows: int = 128) -> int:
    """Guard bytes per side of a [rows, row_bytes] buffer: max(64 KiB, 128 rows), rounded up to 256."""
    g = max(64 << 10, rows * int(row_bytes))
    return (g + ALIGN - 1) // ALIGN * ALIGN


class GuardDamage(AssertionError):
    pass


class Guarded:
    def __init__(self, nbytes: int, guard_bytes: int, body_fill: int = 0xFF, guard_fill: int = OUT_GUARD, device="cpu"):
        nbytes, guard_bytes = int(nbytes), int(guard_bytes)
        if nbytes < 0 or guard_bytes <= 0:
            raise ValueError("Guarded: nbytes >= 0 and guard_bytes > 0")
        self.nbytes, self.guard_bytes, self.guard_fill = nbytes, guard_bytes, int(guard_fill) & 0xFF
        self.raw = torch.empty(guard_bytes + nbytes + guard_bytes + ALIGN, dtype=torch.uint8, device=device)
        self.start = guard_bytes + (-(self.raw.data_ptr() + guard_bytes)) % ALIGN      # body offset inside raw: the body pointer is 256-byte aligned
        self.raw.fill_(self.guard_fill)
        self.body = self.raw[self.start:self.start + nbytes]
        self.body.fill_(int(body_fill) & 0xFF)
        self.low = self.raw[:self.start]
        self.high = self.raw[self.start + nbytes:]
        assert self.low.numel() >= guard_bytes and self.high.numel() >= guard_bytes
        assert (self.raw.data_ptr() + self.start) % ALIGN == 0

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + self.start

    def view(self, dtype, shape):
        return self.body.view(dtype).view(shape)

    def damage(self):
        """[(side, first offset, last offset, count)] of the damaged guards, offsets relative to the body; ONE device -> host transfer."""
        bad_lo = self.low != self.guard_fill
        bad_hi = self.high != self.guard_fill
        big = self.raw.numel()
        pos_lo = torch.arange(self.low.numel(), device=self.raw.device)
        pos_hi = torch.arange(self.high.numel(), device=self.raw.device)
        stats = torch.stack([
            bad_lo.sum(), torch.where(bad_lo, pos_lo, big).min(), torch.where(bad_lo, pos_lo, -1).max(),
            bad_hi.sum(), torch.where(bad_hi, pos_hi, big).min(), torch.where(bad_hi, pos_hi, -1).max(),
        ]).tolist()      # the one sync
        out = []
        if stats[0]:
            out.append(("low", stats[1] - self.start, stats[2] - self.start, stats[0]))
        if stats[3]:
            out.append(("high", self.nbytes + stats[4], self.nbytes + stats[5], stats[3]))
        return out

    def assert_intact(self, name: str = "buffer") -> None:
        d = self.damage()
        if d:
            raise GuardDamage("; ".join(
                f"{name}: {side} guard damaged: {cnt} byte(s), first at body offset {first}, last at body offset {last} (body = {self.nbytes} bytes)"
                for side, first, last, cnt in d))


def guarded_like(t: torch.Tensor, guard_bytes: int, guard_fill: int = IN_GUARD) -> "tuple[Guarded, torch.Tensor]":
    """A guarded copy of an input tensor: (buffer, typed view holding t's values)."""
    t = t.contiguous()
    g = Guarded(t.numel() * t.element_size(), guard_bytes, 0, guard_fill, t.device)
    v = g.view(t.dtype, tuple(t.shape))
    v.copy_(t)
    return g, v
