"""The layout kernels' case tables, without a GPU: the gather cases of tests/layout_cases.py reach every instantiation the launcher
can pick (asked of qllm_gather_describe, the rule the launcher executes, at 256 compute units), the numpy expectations the GPU file
compares against round-trip among themselves, and the entries refuse what they cannot hold before any device work."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import capi_fakes as F
import layout_cases as L
from oracle import ref_cpu as O
from qllm_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = r"""
import json, sys
from qllm_amd import ops
out = {}
for m, k, rows in json.loads(sys.argv[1]):
    try:
        if not rows:
            ops.set_knob("QLLM_GATHER_ROWS", 0)
        out[f"{m},{k},{rows}"] = ops.gather_describe(m, k)
    finally:
        ops.reset_knobs()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def describe_at_256(keys):
    """{(M, K, QLLM_GATHER_ROWS): text} from a child process with QLLM_NUM_CU = 256 (the variable is read once per process)."""
    env = dict(os.environ, QLLM_NUM_CU="256", PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + sys.path))
    got = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(list(keys))], env=env, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr
    out = json.loads(got.stdout.strip().splitlines()[-1])
    return {tuple(int(v) for v in k.split(",")): text for k, text in out.items()}


@pytest.fixture(scope="module")
def described(lib):
    probes = [(m, k, 1) for k in (4096, 8192, 12288, 16384) for m in (64, 1 << 20)]   # the widest K of each cpt, fewest and many rows
    return describe_at_256(list(L.GATHER_CASES) + probes)


# ---- the gather's forms ------------------------------------------------------------------------------------------------------------
def test_the_rule_answers_what_the_table_pins(described):
    for key, want in L.GATHER_CASES.items():
        assert described[key] == want, key


def test_every_required_form_has_a_case():
    forms = [(L.gather_form(text), m, text) for (m, _k, _r), text in L.GATHER_CASES.items()]
    missing = [what for what, rx, cond in L.REQUIRED
               if not any(re.search(rx, text) and (cond is None or cond(f, m)) for f, m, text in forms)]
    assert not missing, missing
    names = [what for what, _rx, _c in L.REQUIRED]
    assert all(f"rows<{r},{c}>" in names for r, c in L.ROWS_FORMS) and all(f"columns<{c}>" in names for c in L.COLUMN_FORMS)
    assert len(L.ROWS_FORMS) == 7 and len(L.COLUMN_FORMS) == 6


def test_the_tables_name_the_instantiations_the_source_builds():
    src = open(os.path.join(os.path.dirname(HERE), "qllm_amd", "csrc", "gather.hip")).read()
    rows = {(int(a), int(b)) for a, b in re.findall(r"launch_rows<(\d+), (\d+)>\(f,", src)}
    assert rows == set(L.ROWS_FORMS)
    cols = re.search(r"kColumnChunks\[\] = \{([^}]*)\}", src).group(1).replace("kMaxChunks", re.search(r"kMaxChunks = (\d+)", src).group(1))
    assert tuple(int(c) for c in cols.split(",")) == L.COLUMN_FORMS
    assert {int(c) for c in re.findall(r"case (\d+): return launch_b<\d+>", src)} | {14} == set(L.COLUMN_FORMS)


def test_no_rows_form_can_pass_the_default_lds_limit(described):
    """REQUIRED asks for a case above 64 KB of dynamic LDS "for each kernel template that can need it": the rows kernel never does --
    its largest request, the widest K of each chunks-per-thread class at any row count, is exactly the limit."""
    for k in (4096, 8192, 12288, 16384):
        for m in (64, 1 << 20):
            f = L.gather_form(described[(m, k, 1)])
            assert f["kernel"] == "rows" and f["cpt"] == k // 4096 and f["lds"] <= L.LDS_DEFAULT_LIMIT, (m, k, f)
    assert L.gather_form(described[(1 << 20, 4096, 1)])["lds"] == L.LDS_DEFAULT_LIMIT


def test_gather_describe_entry(lib):
    buf = C.create_string_buffer(256)
    assert lib.qllm_gather_describe(5, 12, buf, 256) == 0 and buf.value.startswith(b"unsupported (") and b"12" in buf.value
    assert _lib.last_error() == ""
    assert lib.qllm_gather_describe(5, 28680, buf, 256) == 0 and buf.value.startswith(b"unsupported (")
    assert lib.qllm_gather_describe(0, 64, buf, 256) == 0 and buf.value == b"gather nothing (M=0)"
    assert lib.qllm_gather_describe(1, 64, None, 256) == _lib.QLLM_ERR_INVALID and "buf" in _lib.last_error()
    assert lib.qllm_gather_describe(1, 64, buf, 0) == _lib.QLLM_ERR_INVALID
    assert lib.qllm_gather_describe(-1, 64, buf, 256) == _lib.QLLM_ERR_INVALID and "M=-1" in _lib.last_error()
    assert lib.qllm_gather_describe(1, 0, buf, 256) == _lib.QLLM_ERR_INVALID
    # the same words, the same status as the entry that launches (fake pointers: refused before any device work)
    assert lib.qllm_gather_describe(5, 28680, buf, 256) == 0
    assert lib.qllm_gather_columns(F.X, F.PERM, F.Y, 5, 28680, _lib.DT_F16, None) == _lib.QLLM_ERR_UNSUPPORTED
    assert buf.value.decode() == f"unsupported ({_lib.last_error()})"
    assert lib.qllm_gather_columns(F.X, F.PERM, F.Y, -1, 64, _lib.DT_F16, None) == _lib.QLLM_ERR_INVALID and "M=-1" in _lib.last_error()
    assert lib.qllm_gather_describe(3, 8, buf, 256) == 0 and buf.value.startswith(b"gather columns chunks=1 parts=1 rows_per_block=2 grid=2x1")
    from qllm_amd import ops
    assert ops.gather_describe(3, 8) == buf.value.decode()


def test_the_rows_knob_is_settable_and_moves_the_rule(lib):
    from qllm_amd import ops
    try:
        before = ops.gather_describe(64, 64)
        ops.set_knob("QLLM_GATHER_ROWS", 0)
        assert before.startswith("gather rows=2 cpt=1 ") and ops.gather_describe(64, 64).startswith("gather columns chunks=1 ")
        with pytest.raises(_lib.QllmError):
            ops.set_knob("QLLM_GATHER_ROWS", 2)
    finally:
        ops.reset_knobs()
    assert ops.gather_describe(64, 64) == before


def test_gather_inputs():
    for K in (8, 264, 28672):
        for kind in L.PERM_KINDS:
            p = L.gather_perm(K, kind)
            assert p.dtype == np.int32 and p.shape == (K,) and p.min() == 0 and p.max() == K - 1
            assert (len(np.unique(p)) == K) == (kind != "repeats")
        assert (L.gather_perm(K, "reversal") == np.arange(K - 1, -1, -1)).all()
    x = L.gather_x(4099, 264)
    assert (x != L.GATHER_CANARY).all() and (L.gather_x(16390, 64) != L.GATHER_CANARY).all() and len(np.unique(L.gather_x(16390, 64), axis=0)) == 16390
    assert len(np.unique(x, axis=0)) == 4099 and all(len(np.unique(r)) == 264 for r in x[:3])
    assert len(np.unique(L.gather_x(300, 28672)[:, :4], axis=0)) == 300


# ---- the expectations round-trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", range(2, 9))
def test_dequant_expectations(bits):
    cases = L.dequant_cases(bits)
    assert {c[0] for c in cases} == set(L.FLAVOURS) - (set() if bits == 4 else {"awq"})
    assert any(K % g for _f, K, _n, g, _o in cases) and {c[4] for c in cases} == {None, "act_order", "unequal"}
    assert {g for _f, _k, _n, g, _o in cases} >= {8, 16, 32, 64} and any(g == K for _f, K, _n, g, _o in cases)
    for fl, K, N, g, order in cases:
        d = L.make_layer(fl, bits, K, N, g, order)
        w = L.dequant_expect(d)
        assert w.dtype == np.float16 and w.shape == (K, N) and np.isfinite(w).all(), (fl, K, N, g)
        if d["layout"] == "GEMM":
            assert (O.awq_int_weight(d["qweight"], K, N) == d["q"]).all() and (O.awq_int_zeros(d["qzeros"], N) == d["z"]).all()
        else:
            assert (O.gptq_int_weight(d["qweight"], bits, K) == d["q"]).all()
            if d["layout"] == "GPTQ" and d["qzeros"] is not None:
                assert (O.gptq_int_zeros(d["qzeros"], bits, N, d["compat"]) == d["z"]).all()
        if order == "unequal":
            assert len(set(np.bincount(d["g_idx"]))) > 1
        if K * N <= 96 * 288 and order is None and g in (8, K):   # the element-by-element restatement, on the small ones
            if d["qzeros"] is not None:
                assert (O.dequant_loops(d["layout"], d["qweight"], d["scales"], d["qzeros"], None, bits, g, K, d["compat"]).view(np.uint16)
                        == w.view(np.uint16)).all()
        bf = O.f16_to_bf16_bits(w)
        assert (bf.view(np.int16) == torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy()).all()


def test_bf16_rounding_of_every_finite_fp16_value():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    assert (O.f16_to_bf16_bits(h).view(np.int16) == torch.from_numpy(h).to(torch.bfloat16).view(torch.int16).numpy()).all()
    assert (O.f16_to_bf16_bits(h) != (h.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)).any()   # rounding is not truncation


@pytest.mark.parametrize("bits", range(2, 9))
def test_pack_expectations_round_trip(bits):
    top = (1 << bits) - 1
    for K, N in L.PACK_SHAPES:
        grids = L.code_grids(bits, K, N)
        words = [O.pack_along_rows(q, bits) for q in grids]
        for q, w in zip(grids, words):
            assert w.shape == (K * bits // 32, N) and (O.unpack_along_rows(w, bits, K) == q).all()
            assert (O.pack_along_rows(L.with_garbage(q, bits), bits) == w).all()
        both = np.stack([g for g in grids[1:3]])
        assert ((both == 0).any(axis=0) & (both == top).any(axis=0)).all()          # 0 and the top code at every (k, n)
    if bits == 4:
        K, N = L.PACK_SHAPE_AWQ
        for q in L.code_grids(4, K, N):
            w = O.pack_awq(q, q[:1])[0]
            assert w.shape == (K, N // 8) and (O.awq_int_weight(w, K, N) == q).all()


def test_native_expectations_invert():
    for fl, bits, K, N, g in L.native_cases():
        d = L.make_layer(fl, bits, K, N, g)
        nq, ns, nz = L.native_expect(d)
        assert nq.shape == (N // 16, K * bits // 32, 16) and ns.shape == (N // 16, K // g, 16) and (nz is None) == (d["z"] is None)
        q, sc, z = L.native_invert(nq, ns, nz, bits, K, N, d["layout"] == "HQQ")
        assert (q == d["q"]).all() and (sc.view(np.uint16) == d["scales"].view(np.uint16)).all()
        if z is not None:
            assert (z.view(np.uint16) == d["z"].view(np.uint16)).all() if d["layout"] == "HQQ" else (z == d["z"]).all()
    shapes = {(bits, N, fl) for fl, bits, _k, N, _g in L.native_cases()}
    assert {(4, 16, "awq"), (4, 48, "gptq_asym"), (4, 272, "hqq"), (3, 16, "hqq"), (3, 48, "hqq"), (3, 32, "gptq_asym"), (3, 96, "gptq_asym"),
            (3, 224, "gptq_asym")} <= shapes


def test_ort_expectations():
    for K, N, block in L.ORT_SHAPES:
        for zf in (False, True):
            for order in L.ORT_ORDERS:
                c = L.ort_case(K, N, block, zf, order)
                assert c["want"].shape == (N, K) and np.isfinite(c["want"]).all()
                assert (O.ort_int_weight(c["qweight"])[:K] == c["q"]).all()
                if not zf:
                    assert (O.ort_int_zeros(c["qzeros"], N, K // block) == c["z"]).all()
                if order == "unequal" and K // block > 1:
                    assert len(set(np.bincount(c["g_idx"], minlength=K // block))) > 1 and (np.bincount(c["g_idx"], minlength=K // block) > 0).all()
                if order == "permutation":
                    assert (np.bincount(c["g_idx"]) == block).all()


# ---- what the entries refuse, before any device work ----------------------------------------------------------------------------------
def test_refusals(lib):
    p = C.c_void_p
    sizes = [C.c_size_t(0) for _ in range(3)]

    def native(w):
        return (lib.qllm_native_sizes(C.byref(w), *[C.byref(s) for s in sizes]), lib.qllm_repack_native(C.byref(w), p(F.Y), p(F.Y + 4096), p(F.Y + 8192), None))

    # 3-bit packed zero points at N % 32 != 0 (fp16 zero points at the same N are held): the size entry and a native descriptor say
    # unsupported; as a GPTQ source the layer is no valid descriptor at all (N * 3 % 32 != 0 whenever N % 32 != 0)
    w = F.W(bits=3, K=96, N=48, g=32)
    assert native(w) == (_lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_INVALID) and "packed zeros" in _lib.last_error()
    assert lib.qllm_native_sizes(C.byref(w), *[C.byref(s) for s in sizes]) == _lib.QLLM_ERR_UNSUPPORTED and "N % 32" in _lib.last_error()
    w3 = F.W(bits=3, K=96, N=48, g=32, layout=_lib.LAYOUT_NATIVE)
    assert lib.qllm_unpack_native(C.byref(w3), _lib.LAYOUT_GPTQ, p(F.Y), p(F.Y), p(F.Y), None) == _lib.QLLM_ERR_UNSUPPORTED and "N % 32" in _lib.last_error()
    assert lib.qllm_native_sizes(C.byref(F.W(bits=3, K=96, N=48, g=32, layout=_lib.LAYOUT_HQQ)), *[C.byref(s) for s in sizes]) == 0
    assert lib.qllm_native_sizes(C.byref(F.W(bits=3, K=96, N=96, g=32)), *[C.byref(s) for s in sizes]) == 0
    assert (sizes[0].value, sizes[1].value, sizes[2].value) == (9 * 96 * 4, 3 * 96 * 2, 3 * 6 * 8)
    # the native layout at N % 16 != 0
    assert native(F.W(bits=4, K=96, N=40, g=32)) == (_lib.QLLM_ERR_UNSUPPORTED,) * 2 and "N % 16" in _lib.last_error()
    assert lib.qllm_unpack_native(C.byref(F.W(bits=4, K=96, N=40, g=32, layout=_lib.LAYOUT_NATIVE)), _lib.LAYOUT_GPTQ, p(F.Y), p(F.Y), p(F.Y), None) == _lib.QLLM_ERR_UNSUPPORTED
    # AWQ at N % 8 != 0
    awq = F.W(bits=4, K=96, N=20, g=32, layout=_lib.LAYOUT_AWQ_GEMM)
    assert lib.qllm_dequant(C.byref(awq), p(F.Y), _lib.DT_F16, 0, None) == _lib.QLLM_ERR_INVALID and "pack_num" in _lib.last_error()
    assert lib.qllm_repack_native(C.byref(awq), p(F.Y), p(F.Y), p(F.Y), None) == _lib.QLLM_ERR_INVALID
    for entry in (lib.qllm_pack_qweight, lib.qllm_unpack_qweight):
        assert entry(p(F.X), _lib.LAYOUT_AWQ_GEMM, 4, 32, 20, p(F.Y), None) == _lib.QLLM_ERR_INVALID and "N%8" in _lib.last_error()
        assert entry(p(F.X), _lib.LAYOUT_AWQ_GEMM, 3, 32, 16, p(F.Y), None) == _lib.QLLM_ERR_INVALID
    # K * bits % 32 != 0
    for bits, K in ((3, 16), (5, 40), (7, 100), (2, 8)):
        for entry in (lib.qllm_pack_qweight, lib.qllm_unpack_qweight):
            assert entry(p(F.X), _lib.LAYOUT_GPTQ, bits, K, 8, p(F.Y), None) == _lib.QLLM_ERR_INVALID and "multiple of 32" in _lib.last_error()
        assert lib.qllm_dequant(C.byref(F.W(bits=bits, K=K, N=8, g=8)), p(F.Y), _lib.DT_F16, 0, None) == _lib.QLLM_ERR_INVALID
        assert "multiple of 32" in _lib.last_error()
    # packed GPTQ zero points at N * bits % 32 != 0; a symmetric layer of the same shape is a valid descriptor (refused here for its type)
    assert lib.qllm_dequant(C.byref(F.W(bits=3, K=96, N=264, g=32)), p(F.Y), _lib.DT_F16, 0, None) == _lib.QLLM_ERR_INVALID and "packed zeros" in _lib.last_error()
    assert lib.qllm_dequant(C.byref(F.W(bits=3, K=96, N=264, g=32, qzeros=None)), p(F.Y), 7, 0, None) == _lib.QLLM_ERR_INVALID and "out_dtype" in _lib.last_error()
    # the ORT blob: a block that is no multiple of 16, a K that is no multiple of the block
    ort = lambda block, K: lib.qllm_ort_dequantize4bits(p(F.QWEIGHT), p(F.SCALES), p(F.QZEROS), 0, None, block, K, 4, p(F.Y), None)  # noqa: E731
    for block in (8, 24, 40, 0, -16):
        assert ort(block, 240) == _lib.QLLM_ERR_INVALID and "multiple of 16" in _lib.last_error()
    assert ort(32, 48) == _lib.QLLM_ERR_UNSUPPORTED and "block_size" in _lib.last_error()
    # bf16 -> fp16: whole 16-byte pieces
    assert lib.qllm_convert_bf16_to_f16(p(F.X), p(F.Y), 12, None) == _lib.QLLM_ERR_INVALID
