"""The case tables and numpy expectations of the layout kernels: the column gather (csrc/gather.hip), dequant / pack / unpack
(csrc/dequant.hip), the native repack (csrc/native.hip) and the ORT blob (csrc/ortblob.hip).  Shared by test_layout_kernels_cpu.py (the
tables cover every kernel form; the expectations round-trip) and test_layout_kernels_gpu.py (the kernels give these bits).  Every
expectation is built from oracle/ref_cpu.py on the CPU; nothing here calls the library except `gather_form`, which asks the pure-host
qllm_gather_describe."""
import re

import numpy as np

from oracle import ref_cpu as O

# ---- the column gather ------------------------------------------------------------------------------------------------------------
# (M, K, QLLM_GATHER_ROWS) -> what qllm_gather_describe answers with 256 compute units.  The instantiation a case reaches is the
# rule's answer, pinned here; the shapes are the smallest that reach it with a ragged end (M no multiple of the rows per step / block).
GATHER_CASES = {
    (4099, 264, 1): "gather rows=8 cpt=1 grid=512 lds=4224",        # 513 steps over 512 blocks, 3 rows in the last
    (2050, 520, 1): "gather rows=4 cpt=1 grid=512 lds=4160",        # 513 steps, 2 rows in the last
    (65, 4096, 1): "gather rows=2 cpt=1 grid=33 lds=16384",
    (1027, 4096, 1): "gather rows=2 cpt=1 grid=512 lds=16384",      # 514 steps
    (2049, 5120, 1): "gather rows=4 cpt=2 grid=512 lds=40960",      # 513 steps, 1 row in the last
    (67, 8192, 1): "gather rows=2 cpt=2 grid=34 lds=32768",
    (64, 8200, 1): "gather rows=2 cpt=3 grid=32 lds=32800",
    (65, 14336, 1): "gather rows=2 cpt=4 grid=33 lds=57344",
    (64, 16384, 1): "gather rows=2 cpt=4 grid=32 lds=65536",
    (63, 4104, 1): "gather columns chunks=2 parts=2 rows_per_block=2 grid=32x2 lds=16416",
    (63, 11008, 1): "gather columns chunks=4 parts=2 rows_per_block=2 grid=32x2 lds=44032",
    (63, 24576, 1): "gather columns chunks=6 parts=2 rows_per_block=2 grid=32x2 lds=98304",
    (64, 16392, 1): "gather columns chunks=6 parts=2 rows_per_block=2 grid=32x2 lds=65568",
    (63, 28672, 1): "gather columns chunks=8 parts=2 rows_per_block=2 grid=32x2 lds=114688",
    (300, 28672, 1): "gather columns chunks=14 parts=1 rows_per_block=2 grid=150x1 lds=114688",
    (31, 24576, 1): "gather columns chunks=4 parts=4 rows_per_block=2 grid=16x4 lds=98304",
    (15, 28672, 1): "gather columns chunks=2 parts=8 rows_per_block=2 grid=8x8 lds=114688",
    (1, 8, 1): "gather columns chunks=1 parts=1 rows_per_block=1 grid=1x1 lds=32",
    (2, 8, 1): "gather columns chunks=1 parts=1 rows_per_block=2 grid=1x1 lds=32",
    (3, 8, 1): "gather columns chunks=1 parts=1 rows_per_block=2 grid=2x1 lds=32",
    (1, 28672, 1): "gather columns chunks=1 parts=14 rows_per_block=1 grid=1x14 lds=114688",
    (2, 28672, 1): "gather columns chunks=1 parts=14 rows_per_block=2 grid=1x14 lds=114688",
    (3, 28672, 1): "gather columns chunks=1 parts=14 rows_per_block=2 grid=2x14 lds=114688",
    # QLLM_GATHER_ROWS = 0: the row-at-a-time kernel at prefill row counts, the only way to more than 2 rows per block
    (4100, 64, 0): "gather columns chunks=1 parts=1 rows_per_block=4 grid=1025x1 lds=256",
    (8200, 64, 0): "gather columns chunks=1 parts=1 rows_per_block=8 grid=1025x1 lds=256",
    (16390, 64, 0): "gather columns chunks=1 parts=1 rows_per_block=16 grid=1025x1 lds=256",   # 6 rows in the last block
}
ROWS_FORMS = ((8, 1), (4, 1), (2, 1), (4, 2), (2, 2), (2, 3), (2, 4))   # gather_rows_kernel<ROWS, CPT> as built
COLUMN_FORMS = (1, 2, 4, 6, 8, 14)                                      # gather_columns_kernel<CHUNKS> as built
LDS_DEFAULT_LIMIT = 64 * 1024


def gather_form(text):
    """A describe answer as a dict of ints: kernel ("rows" / "columns") and the fields it prints."""
    m = re.fullmatch(r"gather rows=(\d+) cpt=(\d+) grid=(\d+) lds=(\d+)", text)
    if m:
        rows, cpt, grid, lds = map(int, m.groups())
        return dict(kernel="rows", rows=rows, cpt=cpt, grid=grid, lds=lds)
    m = re.fullmatch(r"gather columns chunks=(\d+) parts=(\d+) rows_per_block=(\d+) grid=(\d+)x(\d+) lds=(\d+)", text)
    assert m, text
    chunks, parts, rpb, grid, gy, lds = map(int, m.groups())
    assert gy == parts
    return dict(kernel="columns", chunks=chunks, parts=parts, rows_per_block=rpb, grid=grid, lds=lds)


def _rows(f, M, **want):
    return f["kernel"] == "rows" and all(f[k] == v for k, v in want.items())


def _cols(f, M, **want):
    return f["kernel"] == "columns" and all(f[k] == v for k, v in want.items())


# (what, regular expression over the describe text, a further condition on (form, M) or None): each must be met by a GATHER_CASES entry
REQUIRED = (
    [(f"rows<{r},{c}>", rf"^gather rows={r} cpt={c} ", None) for r, c in ROWS_FORMS]
    + [(f"columns<{c}>", rf"^gather columns chunks={c} ", None) for c in COLUMN_FORMS]
    + [(f"columns<{c}> above the default LDS limit", rf"^gather columns chunks={c} ", lambda f, M: f["lds"] > LDS_DEFAULT_LIMIT) for c in COLUMN_FORMS]
    + [(f"rows_per_block={r}", rf"^gather columns .* rows_per_block={r} ", None) for r in (2, 4, 8, 16)]
    + [("parts > 1 and chunks > 1", r"^gather columns ", lambda f, M: f["parts"] > 1 and f["chunks"] > 1),
       ("rows: more steps than blocks", r"^gather rows=", lambda f, M: -(-M // f["rows"]) > f["grid"]),
       ("rows: ragged last step", r"^gather rows=", lambda f, M: M % f["rows"] != 0),
       ("rows: ragged last step of a grid-stride launch", r"^gather rows=", lambda f, M: M % f["rows"] != 0 and -(-M // f["rows"]) > f["grid"]),
       ("columns: ragged last block", r"^gather columns ", lambda f, M: M % f["rows_per_block"] != 0),
       ("columns: ragged last block of 16 rows", r"^gather columns .* rows_per_block=16 ", lambda f, M: M % 16 != 0)])

PERM_KINDS = ("random", "reversal", "repeats")


def gather_perm(K, kind, seed=0):
    """int32 [K]: a random permutation, the reversal, or a non-injective map with repeats that holds columns 0 and K - 1."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "random":
        p = rng.permutation(K)
    elif kind == "reversal":
        p = np.arange(K)[::-1]
    else:
        p = rng.integers(0, K, size=K)
        p[rng.permutation(K)[:4]] = (0, K - 1, 0, K - 1) if K >= 4 else 0
        p[0], p[K - 1] = K - 1, 0
        assert len(np.unique(p)) < K or K <= 2
    return np.ascontiguousarray(p, dtype=np.int32)


GATHER_CANARY = -1   # int16 0xFFFF (a NaN of both types): the one pattern gather_x never holds


def gather_x(M, K):
    """int16 [M, K] of distinct bit patterns: element (m, k) = (m S + k) mod 65535 -- arange with a row stride S, the first number from
    K + 1 on that has no factor in common with 65535.  A row's K entries differ, no two of the M < 65535 rows are equal (with a stride of
    K, rows 65536 / K apart would be), and 0xFFFF stays free for the canary."""
    assert M < 65535 and K < 65535
    S = K + 1
    while np.gcd(S, 65535) != 1:
        S += 1
    return ((np.arange(M, dtype=np.int64)[:, None] * S + np.arange(K, dtype=np.int64)[None, :]) % 65535).astype(np.uint16).view(np.int16)


# ---- synthetic layers --------------------------------------------------------------------------------------------------------------
FLAVOURS = ("gptq_asym", "gptq_azb1", "gptq_sym", "hqq", "awq")
# (K, N, group sizes): K = 32 x odd throughout; N = 8 (one ragged block), 264 and 520 (ragged last block of 256 threads), 1000 (four
# blocks, the last ragged).  Group sizes 8 and 16 change the group inside one thread's 32-k run; 64 at K = 96 / 160 leaves K % g != 0.
DEQUANT_SHAPES = ((32, 8, (8, 16, 32)), (96, 264, (8, 16, 32, 64, 96)), (160, 1000, (32, 64, 160)), (224, 520, (16, 32, 224)))


def packed_n(N, bits):
    """N as it is, or -- where packed zero points need N * bits % 32 == 0 -- the next multiple of 32 that is no multiple of 256."""
    if (N * bits) % 32 == 0:
        return N
    n = -(-N // 32) * 32
    return n + 32 if n % 256 == 0 else n


def g_idx_of(K, g, kind, rng):
    """None (plain), "act_order" (the plain map permuted: equal group sizes, g_idx[:g] not all zero) or "unequal" (group sizes differ;
    every group is used)."""
    G = -(-K // g)
    if kind is None:
        return None
    if kind == "act_order":
        gi = O.trivial_g_idx(K, g)[rng.permutation(K)]
    else:
        gi = np.concatenate([np.arange(G), rng.integers(0, max(G // 2, 1), size=K - G)])[rng.permutation(K)]
    gi = gi.astype(np.int32)
    if gi[:g].sum() == 0 and G > 1:
        gi[0] = G - 1
    return np.ascontiguousarray(gi)


def make_layer(flavour, bits, K, N, g, g_idx_kind=None, seed=0):
    """A random layer in packed form: dict(layout, bits, K, N, groupsize, q, z (stored integers / fp16 / None), scales, qweight, qzeros,
    g_idx, compat).  Scales span three binades with full mantissas so that each of the three fp16 roundings of W moves bits."""
    rng = np.random.default_rng([seed, bits, K, N, g, FLAVOURS.index(flavour)])
    G = -(-K // g)
    q = rng.integers(0, 1 << bits, size=(K, N), dtype=np.int32)
    q[0, :], q[-1, :] = (1 << bits) - 1, 0
    scales = ((rng.random((G, N)) * 0.07 + 0.01) * rng.choice((-1.0, 1.0), size=(G, N))).astype(np.float16)
    layout, compat, gi = {"hqq": "HQQ", "awq": "GEMM"}.get(flavour, "GPTQ"), int(flavour == "gptq_azb1"), None
    if flavour == "hqq":
        z = (rng.random((G, N)) * ((1 << bits) - 1)).astype(np.float16)
        qweight, qzeros = O.pack_along_rows(q, bits), z
    elif flavour == "awq":
        assert bits == 4 and N % 8 == 0 and K % g == 0
        z = rng.integers(0, 16, size=(G, N), dtype=np.int32)
        qweight, qzeros = O.pack_awq(q, z)
    elif flavour == "gptq_sym":
        z, qweight, qzeros = None, O.pack_along_rows(q, bits), None
        gi = g_idx_of(K, g, g_idx_kind, rng)
    else:
        assert (N * bits) % 32 == 0
        z = rng.integers(0, 1 << bits, size=(G, N), dtype=np.int32)           # the zero points the layer dequantises with
        z[0, 0], z[-1, -1] = 0, (1 << bits) - 1                                  # (azb: stored as z - 1 mod 2^bits, 0 wraps to all ones)
        qweight, qzeros = O.pack_gptq(q, z, bits, compat)
        gi = g_idx_of(K, g, g_idx_kind, rng)
    return dict(layout=layout, bits=bits, K=K, N=N, groupsize=g, q=q, z=z, scales=scales, qweight=qweight, qzeros=qzeros, g_idx=gi,
                compat=compat)


def dequant_expect(d):
    """The oracle's three-rounding fp16 W [K, N] (with g_idx where the layer has one -- the kernel gathers whenever it is given)."""
    return O.dequant(d["layout"], d["qweight"], d["scales"], d["qzeros"], d["g_idx"], d["bits"], d["groupsize"], d["K"], d["compat"])


def dequant_cases(bits):
    """(flavour, K, N, g, g_idx kind) of every dequant case at `bits`."""
    out = []
    for K, N, gs in DEQUANT_SHAPES:
        for g in gs:
            for fl in FLAVOURS:
                if fl == "awq" and (bits != 4 or K % g):
                    continue
                out.append((fl, K, packed_n(N, bits) if fl in ("gptq_asym", "gptq_azb1") else N, g, None))
    for fl in ("gptq_asym", "gptq_sym"):
        n = packed_n(264, bits) if fl == "gptq_asym" else 264
        out += [(fl, 96, n, 32, "act_order"), (fl, 96, n, 16, "unequal"), (fl, 160, n, 64, "unequal")]
    return out


# ---- pack / unpack -----------------------------------------------------------------------------------------------------------------
PACK_SHAPES = ((32, 1), (96, 257))
PACK_SHAPE_AWQ = (32, 8)


def code_grids(bits, K, N, seed=0):
    """int32 [K, N] grids of codes: random, the two checkerboards of 0 and 2^bits - 1 (between them both values sit in every position of
    every word, also where N = 1), all ones."""
    rng = np.random.default_rng([seed, bits, K, N])
    top = (1 << bits) - 1
    board = ((np.arange(K)[:, None] + np.arange(N)[None, :]) & 1).astype(np.int32)
    return [rng.integers(0, top + 1, size=(K, N), dtype=np.int32), board * top, (1 - board) * top, np.full((K, N), top, np.int32)]


def with_garbage(q, bits, seed=0):
    """`q` with random bits -- the sign bit among them -- set above bit `bits`: what the packer must mask away."""
    rng = np.random.default_rng([seed, bits, q.shape[0], q.shape[1], 7])
    junk = rng.integers(0, 1 << 32, size=q.shape, dtype=np.uint64).astype(np.uint32)
    out = (q.astype(np.uint32) | ((junk << np.uint32(bits)) | np.uint32(0x80000000))).view(np.int32)
    assert ((out.view(np.uint32) & np.uint32((1 << bits) - 1)) == q.astype(np.uint32)).all() and (out != q).all()
    return np.ascontiguousarray(out)


# ---- the native layout -------------------------------------------------------------------------------------------------------------
def native_cases():
    """(flavour, bits, K, N, g): 4 bits in the three source layouts at one strip, an odd strip count and a wide N; 3 bits with fp16 zero
    points (N = 16 x odd) and with packed ones (N = 32 x odd); K = 32 (one word row per 8 k) and 96; one group and several; a symmetric layer."""
    out = []
    for K in (32, 96):
        for g in sorted({32, K}):
            out += [(fl, 4, K, N, g) for fl in ("gptq_asym", "awq", "hqq") for N in (16, 48, 272)]
            out += [("hqq", 3, K, N, g) for N in (16, 48)]
            out += [("gptq_asym", 3, K, N, g) for N in (32, 96, 224)]
    return out + [("gptq_sym", 4, 96, 48, 32), ("gptq_sym", 3, 32, 16, 32)]


def native_expect(d):
    """O.native_layout of the layer's integers: (qweight, scales, qzeros or None)."""
    if d["layout"] == "HQQ":
        return O.native_layout(d["q"], d["scales"], d["z"], d["bits"], zeros_f16=True)
    return O.native_layout(d["q"], d["scales"], d["z"], d["bits"])


def native_invert(nq, ns, nz, bits, K, N, zeros_f16):
    """The inverse of O.native_layout in numpy: (q [K, N], scales [G, N], zeros [G, N] or None)."""
    rows = np.asarray(nq).reshape(N // 16, K * bits // 32, 16).transpose(1, 0, 2).reshape(K * bits // 32, N)
    q = O.unpack_along_rows(rows, bits, K)
    G = np.asarray(ns).size // N
    sc = np.asarray(ns).reshape(N // 16, G, 16).transpose(1, 0, 2).reshape(G, N)
    if nz is None:
        return q, sc, None
    if zeros_f16:
        return q, sc, np.asarray(nz).reshape(N // 16, G, 16).transpose(1, 0, 2).reshape(G, N)
    w = np.asarray(nz).view(np.uint32).reshape(N // 16, G, 2).astype(np.uint64)
    pair = w[:, :, 0] | (w[:, :, 1] << np.uint64(32))
    z = np.stack([(pair >> np.uint64(bits * i)) & np.uint64((1 << bits) - 1) for i in range(16)], axis=-1)   # [N/16, G, 16]
    return q, sc, z.transpose(1, 0, 2).reshape(G, N).astype(np.int32)


# ---- the ORT blob ------------------------------------------------------------------------------------------------------------------
ORT_SHAPES = ((16, 1, 16), (96, 3, 32), (48, 5, 16), (384, 7, 128))   # (K, N, block): one thread .. 168; block counts 1, 3, 3, 3 (odd)
ORT_ORDERS = (None, "permutation", "unequal")


def ort_case(K, N, block, zeros_f16, order, seed=0):
    """dict(qweight u8 [N, G, block / 2], scales f16 [N G], qzeros (u8 [N ceil(G / 2)] or f16 [N, G]), g_idx or None, want f16 [N, K])."""
    rng = np.random.default_rng([seed, K, N, block, int(zeros_f16), ORT_ORDERS.index(order)])
    G = K // block
    q = rng.integers(0, 16, size=(K, N), dtype=np.int32)
    q[0, :], q[-1, :] = 15, 0
    s = ((rng.random((G, N)) * 0.07 + 0.01) * rng.choice((-1.0, 1.0), size=(G, N))).astype(np.float16)
    z = (rng.random((G, N)) * 15).astype(np.float16) if zeros_f16 else rng.integers(0, 16, size=(G, N), dtype=np.int32)
    qweight, qzeros, scales = O.pack_ort(q, z, s)
    gi = None
    if order == "permutation":
        gi = O.trivial_g_idx(K, block)[rng.permutation(K)].astype(np.int32)
    elif order == "unequal":
        gi = np.concatenate([np.arange(G), rng.integers(0, max(G - 1, 1), size=K - G)])[rng.permutation(K)].astype(np.int32)
    want = O.dequant_ort(qweight, scales, qzeros, gi, block, K, N)
    return dict(K=K, N=N, block=block, q=q, z=z, s=s, qweight=qweight, scales=scales, qzeros=qzeros, g_idx=gi, want=want)
