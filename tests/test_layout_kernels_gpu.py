"""The kernels that build the layers at load time and permute act-order activations per call -- the column gather (csrc/gather.hip),
dequant / pack / unpack (csrc/dequant.hip), the native repack (csrc/native.hip), the ORT blob (csrc/ortblob.hip) and bf16 -> fp16 -- in
every form their launchers can pick, against the numpy expectations of tests/layout_cases.py.  All of them are integer or
single-rounding operations: every comparison is == on the raw bits."""
import numpy as np
import pytest
import torch

import layout_cases as L
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 1024


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits16(x):
    """a 2-byte tensor / array as int16 numpy"""
    if isinstance(x, torch.Tensor):
        return x.contiguous().view(torch.int16).cpu().numpy()
    return np.ascontiguousarray(x).view(np.int16)


def raw(a):
    """a tensor or an array as numpy unsigned integers of its element size (bf16 has no numpy type of its own)"""
    if isinstance(a, torch.Tensor):
        a = a.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]).cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got, want, what):
    got, want = raw(got), raw(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), (what, f"{int(bad.sum())} of {bad.size} differ, the first at {tuple(int(i) for i in np.argwhere(bad)[0])}")


# ---- the column gather -------------------------------------------------------------------------------------------------------------
def _alloc(shape, dt, canary):
    """An output inside its own buffer, with GUARD elements of the canary before and after it, and pre-filled with it."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), canary, dtype=torch.int16, device=DEV).view(dt)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _bands_intact(buf, canary):
    raw = buf.view(torch.int16)
    return bool((raw[:GUARD] == canary).all()) and bool((raw[-GUARD:] == canary).all())


@pytest.fixture(scope="module")
def cus():
    from qllm_amd import _lib
    return _lib.device_info(0)["compute_units"]


@pytest.mark.parametrize("M,K,rows_knob", list(L.GATHER_CASES), ids=[f"{m}x{k}" + ("" if r else "-rows0") for m, k, r in L.GATHER_CASES])
def test_gather_every_form(M, K, rows_knob, cus):
    from qllm_amd import _lib, ops
    lib = _lib.load()
    x16 = L.gather_x(M, K)
    try:
        if not rows_knob:
            ops.set_knob("QLLM_GATHER_ROWS", 0)
        form = ops.gather_describe(M, K)
        print(f"gather M={M} K={K} QLLM_GATHER_ROWS={rows_knob} on {cus} CUs: {form}")
        if cus == 256:
            assert form == L.GATHER_CASES[(M, K, rows_knob)]
        assert (x16 != L.GATHER_CANARY).all()
        xs = {dt: t(x16).view(dt) for dt in (torch.float16, torch.bfloat16)}
        for kind in L.PERM_KINDS:
            perm = L.gather_perm(K, kind, seed=M)
            want = x16[:, perm]
            perm_d = t(perm)
            for dt, code in ((torch.float16, _lib.DT_F16), (torch.bfloat16, _lib.DT_BF16)):
                x = xs[dt]
                buf, out = _alloc((M, K), dt, L.GATHER_CANARY)
                _lib.check(lib.qllm_gather_columns(x.data_ptr(), perm_d.data_ptr(), out.data_ptr(), M, K, code, torch.cuda.current_stream().cuda_stream))
                torch.cuda.synchronize()
                assert _bands_intact(buf, L.GATHER_CANARY), (kind, dt, "a store outside out")
                got = bits16(out)
                assert not (got == L.GATHER_CANARY).any(), (kind, dt, f"{int((got == L.GATHER_CANARY).sum())} elements never written")
                same(got, want, (kind, dt))
                if kind == "random" and dt == torch.float16:
                    same(ops.gather_columns(x, perm_d), want, "ops.gather_columns")
        for dt, x in xs.items():
            same(x, x16, (dt, "x was written"))
    finally:
        ops.reset_knobs()


# ---- dequant -----------------------------------------------------------------------------------------------------------------------
def _descriptor(d):
    from qllm_amd import ops
    qz = None if d["qzeros"] is None else t(d["qzeros"])
    gi = None if d["g_idx"] is None else t(d["g_idx"])
    return ops.make_weight(d["layout"], t(d["qweight"]), t(d["scales"]), qz, gi, None, d["K"], d["N"], d["groupsize"], d["bits"], d["compat"])


@pytest.mark.parametrize("bits", range(2, 9))
def test_dequant_every_layout_and_output(bits):
    """W = fp16(fp16(s q) - fp16(z s)), bit for bit; the bf16 output is that fp16 value rounded to nearest even."""
    from qllm_amd import ops
    for fl, K, N, g, order in L.dequant_cases(bits):
        d = L.make_layer(fl, bits, K, N, g, order)
        w16 = L.dequant_expect(d)
        wbf = O.f16_to_bf16_bits(w16)
        w, keep = _descriptor(d)
        for dt, want in ((torch.float16, w16), (torch.bfloat16, wbf)):
            same(ops.dequant(w, DEV, dt, False), want, (fl, K, N, g, order, dt))
            same(ops.dequant(w, DEV, dt, True), want.T, (fl, K, N, g, order, dt, "transposed"))
        del keep


# ---- pack / unpack -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", range(2, 9))
def test_pack_and_unpack(bits):
    from qllm_amd import ops
    shapes = [("GPTQ", K, N) for K, N in L.PACK_SHAPES] + ([("GEMM",) + L.PACK_SHAPE_AWQ] if bits == 4 else [])
    for layout, K, N in shapes:
        for i, q in enumerate(L.code_grids(bits, K, N)):
            want = O.pack_along_rows(q, bits) if layout == "GPTQ" else O.pack_awq(q, q[:1])[0]
            same(ops.pack_qweight(t(q), layout, bits), want, (layout, K, N, i, "pack"))
            same(ops.pack_qweight(t(L.with_garbage(q, bits)), layout, bits), want, (layout, K, N, i, "pack, bits set above the code"))
            same(ops.unpack_qweight(t(want), layout, bits, K, N), q, (layout, K, N, i, "unpack"))


# ---- the native layout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (3, 4))
def test_native_repack_and_unpack(bits):
    from qllm_amd import ops
    for fl, b, K, N, g in L.native_cases():
        if b != bits:
            continue
        d = L.make_layer(fl, bits, K, N, g)
        what = (fl, bits, K, N, g)
        w, keep = _descriptor(d)
        nw, nkeep = ops.repack_native(w, keep)
        for got, want, name in zip(nkeep[:3], L.native_expect(d), ("qweight", "scales", "qzeros")):
            assert (got is None) == (want is None), (what, name)
            if want is not None:
                same(got, want.reshape(-1), (what, "native", name))
        back = ops.unpack_native(nw, nkeep, d["layout"])
        for got, want, name in zip(back, (d["qweight"], d["scales"], d["qzeros"]), ("qweight", "scales", "qzeros")):
            assert (got is None) == (want is None), (what, name)
            if want is not None:
                same(got, want, (what, "back to " + d["layout"], name))
        if bits == 4 and fl in ("gptq_asym", "awq"):    # GPTQ <-> AWQ through the native form: the other layout's buffers of the same integers
            other = "GEMM" if fl == "gptq_asym" else "GPTQ"
            qw, qz = O.pack_awq(d["q"], d["z"]) if other == "GEMM" else O.pack_gptq(d["q"], d["z"], 4)
            got = ops.unpack_native(nw, nkeep, other)
            same(got[0], qw, (what, "to " + other, "qweight"))
            same(got[1], d["scales"], (what, "to " + other, "scales"))
            same(got[2], qz, (what, "to " + other, "qzeros"))


# ---- the ORT blob ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,block", L.ORT_SHAPES)
def test_ort_blob_dequant(K, N, block):
    from qllm_amd import ops
    for zf in (False, True):
        for order in L.ORT_ORDERS:
            c = L.ort_case(K, N, block, zf, order)
            gi = None if c["g_idx"] is None else t(c["g_idx"])
            got = ops.ort_dequantize4bits(t(c["qweight"]), t(c["scales"]), t(c["qzeros"]), gi, block, K, N)
            same(got, c["want"], (K, N, block, zf, order))


# ---- bf16 -> fp16 ------------------------------------------------------------------------------------------------------------------
def test_bf16_to_f16_on_every_bit_pattern():
    """All 65536 bf16 values in one call: beyond fp16's range (-> inf), its subnormals, the ties, both zeros, inf and NaN."""
    from qllm_amd import _lib
    src = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    want = src.to(torch.float16)
    dst = torch.full((65536,), -1, dtype=torch.int16, device=DEV).view(torch.float16)
    src_d = src.to(DEV)
    _lib.check(_lib.load().qllm_convert_bf16_to_f16(src_d.data_ptr(), dst.data_ptr(), 65536, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = dst.cpu()
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    assert torch.equal(nan_w, nan_g), f"NaN at {int((nan_w != nan_g).sum())} other patterns"
    bad = (got.view(torch.int16) != want.view(torch.int16)) & ~nan_w
    assert not bool(bad.any()), f"{int(bad.sum())} patterns differ, the first: bf16 0x{int(torch.nonzero(bad)[0]):04x}"
    assert int(nan_w.sum()) == 2 * 127 and bool(torch.isinf(want).sum() > 2)   # the table holds what it is meant to


# ---- capture -----------------------------------------------------------------------------------------------------------------------
def test_the_family_in_a_graph_replays_bit_equal():
    from qllm_amd import ops
    M, K = 65, 4096
    x, perm = t(L.gather_x(M, K)).view(torch.float16), t(L.gather_perm(K, "random"))
    d = L.make_layer("gptq_asym", 3, 96, 288, 32)
    n = L.make_layer("gptq_asym", 4, 96, 48, 32)
    (w, keep), (wn, keepn) = _descriptor(d), _descriptor(n)

    def run():
        return [ops.gather_columns(x, perm), ops.dequant(w, DEV, torch.bfloat16, True)] + [b for b in ops.repack_native(wn, keepn)[1][:3]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [o.clone() for o in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same(eager[0], L.gather_x(M, K)[:, L.gather_perm(K, "random")], "gather")
    same(eager[1], O.f16_to_bf16_bits(L.dequant_expect(d)).T, "dequant")
    for got, want in zip(eager[2:], L.native_expect(n)):
        same(got, want.reshape(-1), "repack")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            same(o, e, "replay")
