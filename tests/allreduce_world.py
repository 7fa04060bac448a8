"""A world of W tensor-parallel ranks inside ONE process, for the one-shot all-reduce (csrc/comm.hip) and the fused GEMV + all-reduce
(csrc/strip1_body.inc, AR): the staging protocol is plain device memory -- slots, flags, an epoch and a ticket -- so a test can give a
rank exactly what its peers would have written, launch that one rank and check every byte it wrote.

Host part (no GPU): the staging buffer's layout, the expected sum (fp32, rank order onto 0.0f, ONE rounding to the activation type) and
the vectors whose sum tells a wrong order or a narrow accumulator apart.  Device part: `World`."""
import ctypes as C

import numpy as np
import torch

MAX_WORLD = 16                       # kCommMaxWorld (csrc/kernels.hpp)
CTL_BYTES = (2 * MAX_WORLD + 2) * 4  # CommCtl: flag[2][16], epoch, ticket
GUARD = 4096                         # bytes of 0xFF on both sides of every staging buffer


class Layout:
    """Byte offsets inside one rank's staging buffer: [2 parities][world][slot_bytes] payload | CommCtl."""

    def __init__(self, world, slot_bytes):
        assert 1 <= world <= MAX_WORLD and slot_bytes % 16 == 0
        self.world, self.slot_bytes = world, slot_bytes
        self.payload = 2 * world * slot_bytes
        self.epoch = self.payload + 2 * MAX_WORLD * 4
        self.ticket = self.epoch + 4
        self.total = self.payload + CTL_BYTES

    def slot(self, parity, r):
        return (parity * self.world + r) * self.slot_bytes

    def flag(self, parity, r):
        return self.payload + (parity * MAX_WORLD + r) * 4

    def region(self, off):
        """what lives at byte `off` (for messages)"""
        if off < 0 or off >= self.total:
            return "guard band %s the buffer (%+d)" % (("before", off) if off < 0 else ("after", off - self.total))
        if off < self.payload:
            s, at = divmod(off, self.slot_bytes)
            return "slot[%d][%d] byte %d" % (s // self.world, s % self.world, at)
        if off < self.epoch:
            f = (off - self.payload) // 4
            return "flag[%d][%d]" % (f // MAX_WORLD, f % MAX_WORLD)
        return "epoch" if off < self.ticket else "ticket"


# ---- the expected bits ------------------------------------------------------------------------------------------------------------------

def widen(bits, dtype):
    """uint16 bit patterns of `dtype` ("f16" / "bf16") -> the same values in fp32 (exact)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def narrow(acc, dtype):
    """fp32 -> the uint16 bit patterns of `dtype`, round to nearest even (f32_to_bf16 of csrc/common.hpp; the hardware's fp16 conversion)"""
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return acc.astype(np.float16).view(np.uint16)
    return torch.from_numpy(acc).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def expected_sum(vectors, dtype, order=None):
    """What every rank must hold after the all-reduce of `vectors` (one uint16 array per rank): widened to fp32, added one at a time in
    rank order onto 0.0f, rounded once."""
    acc = np.zeros(len(vectors[0]), dtype=np.float32)
    for r in (range(len(vectors)) if order is None else order):
        acc = acc + widen(vectors[r], dtype)
    return narrow(acc, dtype)


def narrow_accumulator_sum(vectors, dtype):
    """The same sum with a 16-bit accumulator (rounded after every addition): what expected_sum must NOT equal on mixed_vectors"""
    acc = np.zeros(len(vectors[0]), dtype=np.float32)
    for v in vectors:
        acc = widen(narrow(acc + widen(v, dtype), dtype), dtype)
    return narrow(acc, dtype)


def mixed_vectors(world, n, dtype, seed):
    """One vector of n elements per rank, magnitudes mixed inside every element.  Three quarters of the elements (worlds of three and
    more): two ranks, drawn per element, hold +L and exactly -L (|L| about 1e3 in fp16, 3e4 in bf16: fp32 then keeps about 1e-4 / 4e-3 of
    what is added to them), all others about 1e-2 -- the sum is the small ranks' sum, and which of their low bits survive depends on where
    in the order the large pair sits and on the accumulator's width.  The remaining elements: every rank about 1e3, 1 or 1e-2 at random.
    Finite, no negative zero (a world of one then returns its input bit for bit)."""
    rng = np.random.default_rng(seed)
    big = 1e3 if dtype == "f16" else 3e4
    cols = np.arange(n)
    vals = rng.standard_normal((world, n)).astype(np.float32) * np.float32(1e-2)
    free = rng.random(n) < 0.25 if world >= 3 else np.ones(n, dtype=bool)
    scale = np.array([big, 1.0, 1e-2], dtype=np.float32)[rng.integers(0, 3, size=(world, n))]
    vals[:, free] = (rng.standard_normal((world, n)).astype(np.float32) * scale)[:, free]
    bits = np.stack([narrow(v, dtype) for v in vals])
    if world >= 3:
        a = rng.integers(0, world, size=n)
        b = (a + 1 + rng.integers(0, world - 1, size=n)) % world
        large = narrow((rng.uniform(0.5, 1.0, size=n) * big * rng.choice([-1.0, 1.0], size=n)).astype(np.float32), dtype)
        pair = ~free
        bits[a[pair], cols[pair]] = large[pair]
        bits[b[pair], cols[pair]] = large[pair] ^ np.uint16(0x8000)
    bits[bits == 0x8000] = 0
    assert np.isfinite(widen(bits.reshape(-1), dtype)).all()
    return [np.ascontiguousarray(v) for v in bits]


def cancelling_large(n, dtype, seed):
    """n large values L (either sign) for a rank whose neighbour holds -L, so large that fp32's grid at L is about the last bit of an
    output of magnitude 1 in `dtype`: |L| in 8192..16384 for fp16 (grid 2^-10 = y's ulp), 2^17..2^18 for bf16 (grid 2^-6, y's ulp 2^-7)"""
    rng = np.random.default_rng(seed)
    lo = 8192.0 if dtype == "f16" else 2.0 ** 17
    return narrow((rng.uniform(1.0, 2.0, size=n) * lo * rng.choice([-1.0, 1.0], size=n)).astype(np.float32), dtype)


# ---- the world ---------------------------------------------------------------------------------------------------------------------------

class _DeviceBytes:
    """nbytes of device memory at ptr as torch.as_tensor takes it (zero-copy)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def bits_of(t):
    """the uint16 bit patterns of an fp16 / bf16 device tensor, on the host"""
    return t.contiguous().view(torch.int16).reshape(-1).cpu().numpy().view(np.uint16)


class World:
    """W staging buffers (qllm_comm_alloc memory wrapped as tensors; 0xFF guards, 0xFF slots, a zero control block), ONE pointer table
    and ONE status word shared by all ranks, and a shadow copy of every buffer that follows what the protocol says a launch writes.

        e, parity = world.begin(rho, vectors, real)     # presets the ranks that have not pushed, then the pre-launch checks
        ... one launch of rank rho (world.oneshot / world.fused) ...
        world.finish(rho, e, parity, pushed_bits)       # synchronises; status, epoch, ticket, slots, flags, every other byte

    No launch is a probe: begin() reads rank rho's control block back on the host and asserts that every flag the kernel will wait for
    already carries this call's epoch, that the ticket is armed and that the table holds the W buffers."""

    def __init__(self, lib, world, slot_bytes, device="cuda:0"):
        from qllm_amd import _lib as L
        self.L, self.lib, self.dev = L, lib, device
        self.lay = Layout(world, slot_bytes)
        self.W = world
        assert lib.qllm_comm_buffer_bytes(world, slot_bytes) == self.lay.total
        self._ptrs, self.raw, self.shadow, self.base = [], [], [], []
        size = GUARD + self.lay.total + GUARD
        for _ in range(world):
            p = C.c_void_p()
            L.check(lib.qllm_comm_alloc(size, C.byref(p)))
            self._ptrs.append(p)
            raw = torch.as_tensor(_DeviceBytes(p.value, size), device=device)
            assert raw.data_ptr() == p.value and raw.dtype == torch.uint8 and raw.numel() == size
            raw.fill_(0xFF)
            raw[GUARD + self.lay.payload:GUARD + self.lay.total] = 0
            self.raw.append(raw)
            self.shadow.append(raw.clone())
            self.base.append(p.value + GUARD)
            assert self.base[-1] % 256 == 0
        self.table = torch.tensor(self.base, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.rounds = 0            # epochs every rank has completed, as the test believes

    def close(self):
        torch.cuda.synchronize()
        self.raw, self.shadow = [], []
        for p in self._ptrs:
            self.lib.qllm_comm_free(p)
        self._ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- writes of the test itself: into the buffer and its shadow alike
    def _poke(self, q, off, data_u8):
        for t in (self.raw[q], self.shadow[q]):
            t[GUARD + off:GUARD + off + data_u8.numel()] = data_u8

    def _poke_u32(self, q, off, value):
        for t in (self.raw[q], self.shadow[q]):
            t[GUARD + off:GUARD + off + 4].view(torch.int32).fill_(value)

    def ctl(self, q):
        """rank q's control block on the host: int32[34] = flag[2][16], epoch, ticket"""
        lo = GUARD + self.lay.payload
        return self.raw[q][lo:lo + CTL_BYTES].view(torch.int32).cpu().numpy()

    def preset(self, rho, r, e, vec):
        """what rank r's push of epoch e leaves in rank rho's buffer: its vector at slot[parity][r], then flag[parity][r] = e"""
        parity = e & 1
        self._poke(rho, self.lay.slot(parity, r), vec.contiguous().view(torch.uint8).reshape(-1))
        self._poke_u32(rho, self.lay.flag(parity, r), e)

    def begin(self, rho, vectors, real=()):
        """`vectors[r]`: the device tensor rank r pushes this round (fp16 / bf16, n elements); `real`: the ranks whose push into rank
        rho's buffer came from a launch of this round (the test must not write those)."""
        lay = self.lay
        e = int(self.ctl(rho)[2 * MAX_WORLD]) + 1
        assert e == self.rounds + 1, ("the ranks' epochs have left lockstep", rho, e, self.rounds)
        parity = e & 1
        for r in range(self.W):
            if r != rho and r not in real:
                assert vectors[r].numel() * 2 <= lay.slot_bytes
                self.preset(rho, r, e, vectors[r])
        torch.cuda.synchronize()
        # ---- nothing is launched unless every wait of the kernel is already satisfied
        ctl = self.ctl(rho)
        for r in range(self.W):
            assert r == rho or int(ctl[parity * MAX_WORLD + r]) == e, ("flag not set before the launch", rho, r, e, int(ctl[parity * MAX_WORLD + r]))
        assert int(ctl[2 * MAX_WORLD + 1]) == 0, ("ticket not armed before the launch", rho, e)
        assert self.table.cpu().tolist() == self.base, "the pointer table does not hold the world's buffers"
        assert int(self.status.item()) == 0, ("status word set before the launch", rho, e)
        return e, parity

    def end_round(self):
        """every rank of the world (every rank the test runs) has made this round's call"""
        self.rounds += 1

    def oneshot(self, rho, t):
        """qllm_allreduce_oneshot of rank rho, in place on t, on the current stream"""
        dt = self.L.DT_BF16 if t.dtype == torch.bfloat16 else self.L.DT_F16
        rc = self.lib.qllm_allreduce_oneshot(self.table.data_ptr(), rho, self.W, t.data_ptr(), t.numel(), dt, self.lay.slot_bytes,
                                             self.status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, self.L.last_error())

    def fused(self, rho, w, x, y):
        """qllm_linear_forward_allreduce of rank rho on the current stream"""
        dt = self.L.DT_BF16 if x.dtype == torch.bfloat16 else self.L.DT_F16
        rc = self.lib.qllm_linear_forward_allreduce(C.byref(w), x.data_ptr(), y.data_ptr(), 1, dt, self.table.data_ptr(), rho, self.W,
                                                    self.lay.slot_bytes, self.status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, self.L.last_error())

    def finish(self, rho, e, parity, pushed):
        """After rank rho's launch of epoch e: `pushed` (device tensor) is the vector it had to push."""
        lay = self.lay
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0, f"epoch {e} rank {rho} of {self.W}: the kernel gave up waiting for a flag (status 1)"
        ctl = self.ctl(rho)
        assert int(ctl[2 * MAX_WORLD]) == e, ("epoch", rho, e, int(ctl[2 * MAX_WORLD]))
        assert int(ctl[2 * MAX_WORLD + 1]) == 0, ("ticket not re-armed", rho, e, int(ctl[2 * MAX_WORLD + 1]))
        data = pushed.contiguous().view(torch.uint8).reshape(-1)
        for q in range(self.W):          # what the protocol says the launch wrote, into the shadows ...
            lo = GUARD + lay.slot(parity, rho)
            self.shadow[q][lo:lo + data.numel()] = data
            self.shadow[q][GUARD + lay.flag(parity, rho):GUARD + lay.flag(parity, rho) + 4].view(torch.int32).fill_(e)
        self.shadow[rho][GUARD + lay.epoch:GUARD + lay.epoch + 4].view(torch.int32).fill_(e)
        for q in range(self.W):          # ... and every byte of every buffer, guards included, must be its shadow
            if not torch.equal(self.raw[q], self.shadow[q]):
                bad = torch.nonzero(self.raw[q] != self.shadow[q]).reshape(-1)
                first = int(bad[0]) - GUARD
                raise AssertionError(f"epoch {e} rank {rho} of {self.W}: buffer {q} differs from the protocol in {bad.numel()} bytes, first at "
                                     f"{lay.region(first)} (the push is slot[{parity}][{rho}] bytes 0..{data.numel() - 1}): "
                                     f"{int(self.raw[q][bad[0]])} instead of {int(self.shadow[q][bad[0]])}")
