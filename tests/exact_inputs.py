"""Layers and activations on which every kernel route has exactly ONE correct answer (tests/test_exact_routes_cpu.py, _gpu.py).

The layer (`synth_exact`): q uniform in [0, 2^bits), integer zero points (packed, or integer-valued halves for HQQ), scales that are
powers of two 2^-9 .. 2^-6 drawn per (group, column), a bias in multiples of 2^-6.  The oracle's W -- three fp16 roundings -- is then
exactly s (q - z), and so is the strips' unrounded W: every route's contract names the same number.

Pass 1 (`OneHot`): a seeded permutation of 0..K-1 dealt out M rows per launch, one non-zero of 1 / -1 / 2 per row.  y = x_k W[k, :] +
bias: a read-back of every weight, its zero point and its scale through the route's own fragment layout, exact in fp16 with a bias and
in bf16 without one.  Pass 2 (`sum_rows` on `column_scaled(layer)`): nnz = 2^p / (2^bits - 1) entries of +-1 per row (K / 2 at most), one in each
of nnz slices of K, p = 11 for fp16 and 8 for bf16 results: every partial sum in any order is an integer below 2^p times the column's scale.

Nothing here is assumed: `layer_w64` and `representable` check on the CPU, from the oracle alone, that W is s (q - z) and that the
float64 expectation survives the output type unchanged.  The comparison (`mismatches`) is ==, element for element.  Pure numpy / torch
CPU / oracle.ref_cpu: nothing of the library."""
import numpy as np
import torch

from oracle import ref_cpu as O

VALUES = (1.0, -1.0, 2.0)                 # pass 1's non-zeros
EXPONENTS = (-9, -6)                      # scales are 2^e, e uniform in this closed range
SUM_BITS = {"f16": 11, "bf16": 8}         # pass 2: sums stay below 2^p scale units (the significand of the result type)
MIN_NNZ = 4                               # pass 2 is not run with fewer non-zeros than this
TORCH_DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}


def synth_exact(layout, bits, g, K, N, zero_kind="asym", act_order=False, bias=False, seed=0):
    """gpu_util.synth's dict (the same packed form, the same draws in the same order) for an exactly representable layer, plus the
    integers it was packed from: "q" uint8 [K, N] and "z" float32 [G, N]."""
    rng = np.random.default_rng(seed)
    G = (K + g - 1) // g
    q = rng.integers(0, 2 ** bits, size=(K, N), dtype=np.int32)
    scales = (2.0 ** rng.integers(EXPONENTS[0], EXPONENTS[1] + 1, size=(G, N))).astype(np.float16)
    if layout == "HQQ":
        zeros = rng.integers(0, 2 ** bits, size=(G, N)).astype(np.float16)
        qweight, qzeros = O.pack_along_rows(q, bits), zeros
    else:
        zeros = (np.full((G, N), 2 ** (bits - 1), np.int32) if zero_kind == "sym"
                 else rng.integers(0, 2 ** bits, size=(G, N), dtype=np.int32))
        qweight, qzeros = (O.pack_awq(q, zeros) if layout == "GEMM" else O.pack_gptq(q, zeros, bits))
    g_idx = O.trivial_g_idx(K, g)
    if act_order:
        g_idx = g_idx[rng.permutation(K)].astype(np.int32)
        if g_idx[:g].sum() == 0:
            g_idx[0] = G - 1
    b = (rng.integers(-64, 65, size=N) * 2.0 ** -6).astype(np.float16) if bias else None
    return dict(layout=layout, bits=bits, groupsize=g, K=K, N=N, qweight=qweight, qzeros=qzeros, scales=scales, g_idx=g_idx, bias=b,
                compat=0, q=q.astype(np.uint8), z=zeros.astype(np.float32))


def column_scaled(d, seed=0):
    """Pass 2's layer: `d` with scales that vary by column only (constant over the groups) and no bias; the same q and zero points."""
    e = np.random.default_rng(seed).integers(EXPONENTS[0], EXPONENTS[1] + 1, size=(1, d["N"]))
    return dict(d, scales=np.ascontiguousarray(np.broadcast_to(2.0 ** e, d["scales"].shape)).astype(np.float16), bias=None)


def oracle_w(d):
    """the reference's W [K, N] fp16 (with g_idx for an act-order layer)"""
    gi = d["g_idx"] if (d["layout"] == "GPTQ" and O.is_act_order(d["g_idx"], d["groupsize"])) else None
    return O.dequant(d["layout"], d["qweight"], d["scales"], d["qzeros"], gi, d["bits"], d["groupsize"], d["K"], d.get("compat", 0))


def exact_w(d):
    """s (q - z) in float64 from the integers the layer was packed from: torch [K, N]"""
    gi = torch.from_numpy(d["g_idx"].astype(np.int64))
    q, z, s = torch.from_numpy(d["q"]), torch.from_numpy(d["z"]), torch.from_numpy(d["scales"])
    return (q.double() - z.double()[gi]) * s.double()[gi]


def layer_w64(d):
    """PRECONDITION 1: the oracle's W, through its three fp16 roundings, is s (q - z).  Returns it in float64 (torch [K, N])."""
    w = torch.from_numpy(oracle_w(d)).double()
    want = exact_w(d)
    bad = int((w != want).sum())
    assert bad == 0, f"construction error: the oracle's W differs from s (q - z) in {bad} elements"
    return w


def representable(y64, dtype):
    """PRECONDITION 2: the float64 expectation survives -> `dtype` -> float64 unchanged.  Returns it in `dtype`."""
    y = y64.to(TORCH_DTYPE[dtype])
    bad = int((y.double() != y64).sum())
    assert bad == 0, f"construction error: {bad} expected values are not representable in {dtype}"
    return y


# ---- pass 1: read-back -------------------------------------------------------------------------------------------------------------
class OneHot:
    """A seeded permutation of 0..K-1 dealt out M rows per launch: launch j's row i has its one non-zero at k = perm[j M + i], of value
    val[k]; the rows of the last launch past the end of the permutation are zero (k = -1: y = bias)."""

    def __init__(self, K, M, seed):
        rng = np.random.default_rng(seed)
        self.K, self.M = K, M
        self.perm = rng.permutation(K)
        self.val = rng.choice(np.asarray(VALUES), size=K)
        self.launches = -(-K // M)

    def ks(self, first, count=1):
        """the k of every row of `count` launches from launch `first` on (-1: a zero row)"""
        ks = np.full(count * self.M, -1, np.int64)
        seg = self.perm[first * self.M:(first + count) * self.M]
        ks[:len(seg)] = seg
        return ks

    def x(self, ks):
        x = torch.zeros(len(ks), self.K, dtype=torch.float32)
        live = np.flatnonzero(ks >= 0)
        x[torch.from_numpy(live), torch.from_numpy(ks[live])] = torch.from_numpy(self.val[ks[live]]).float()
        return x

    def expected(self, w64, bias, ks):
        """float64 [len(ks), N]: val[k] W[k, :] + bias"""
        live = torch.from_numpy(ks >= 0)
        kk = torch.from_numpy(np.maximum(ks, 0))
        y = w64[kk] * (torch.from_numpy(self.val)[kk] * live).unsqueeze(1)
        if bias is not None:
            y = y + torch.from_numpy(bias).double()
        return y


# ---- pass 2: sums ------------------------------------------------------------------------------------------------------------------
def sum_nnz(bits, dtype, K):
    """non-zeros per row: as many as keep every sum below 2^p scale units, and no more than K / 2 (slices of two k at least)"""
    return min(2 ** SUM_BITS[dtype] // (2 ** bits - 1), K // 2)


def slice_edges(K, nnz):
    return np.arange(nnz + 1) * K // nnz


def sum_rows(K, rows, nnz, seed):
    """float32 [rows, K]: per row one entry of +-1 at a seeded place in each of `nnz` slices of K"""
    rng = np.random.default_rng(seed)
    edges = slice_edges(K, nnz)
    pos = rng.integers(edges[:-1], edges[1:], size=(rows, nnz))
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(rows, nnz))
    x = torch.zeros(rows, K, dtype=torch.float32)
    x.scatter_(1, torch.from_numpy(pos), torch.from_numpy(sign))
    return x


def sum_expected(w64, x):
    return x.double() @ w64


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def mismatches(got, want, limit=6):
    """`got == want` numerically (-0 equals +0, a NaN equals nothing) over two tensors of one shape on any device: the number of bad
    elements and the first few (row, column, got, want) -- only those leave the device."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    count = int(bad.sum())
    if count == 0:
        return 0, []
    at = bad.nonzero()[:limit]
    g, w = got[at[:, 0], at[:, 1]].double().cpu().tolist(), want[at[:, 0], at[:, 1]].double().cpu().tolist()
    return count, [(int(i), int(n), a, b) for (i, n), a, b in zip(at.cpu().tolist(), g, w)]


def describe(d, ks, count, first):
    """the failure text: the count and the first few (k, n, got, want, q, z, s); k = -1 with the row number where a row has no single k"""
    out = [f"{count} bad elements; (k, n, got, want, q, z, s):"]
    for i, n, got, want in first:
        k = int(ks[i]) if ks is not None else -1
        if k >= 0:
            grp = int(d["g_idx"][k])
            out.append(f"  ({k}, {n}, {got!r}, {want!r}, {int(d['q'][k, n])}, {float(d['z'][grp, n])}, {float(d['scales'][grp, n])})")
        else:
            out.append(f"  (row {i}: -1, {n}, {got!r}, {want!r}, -, -, -)")
    return "\n".join(out)
