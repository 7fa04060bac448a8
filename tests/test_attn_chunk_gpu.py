"""-m gpu: ops.attn_chunk (qllm_attn_chunk, csrc/attn_chunk.hip) on the device: a few query rows behind a cache of about six key tiles, so
that several splits exist at batch 1..3.  The reference is attn_prefill_cases.oracle (float64), the tolerance attn_prefill_cases.bound as
it stands (P is rounded once, relative to a split's running maximum: its terms hold unchanged).  Tile, chunk and splits are read from
ops.attn_chunk_describe, never written here."""
import functools
import re

import pytest
import torch

from attn_prefill_cases import DIMS, DTYPES, GROUPS, bound, fp32_error, left_padded, oracle, selection, selection_expected

from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LMAX = 64 * 5 + 7
# q_len per (Hq, Hkv): S = 2; R = G * S no multiple of 32 -- (7, 1) at 3, (8, 2) at 9: a second row tile that is mostly padding --; exactly
# two row tiles; R = 128 with (8, 1) at 16
Q_LENS = {(1, 1): (2, 16), (8, 2): (2, 9, 16), (7, 1): (3, 16), (8, 1): (2, 16)}
COUNTER_BYTES = 16384


def tag(dtype):
    return str(dtype)[6:]


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def geometry(b, hq, hk, d, s, lmax=LMAX):
    text = ops.attn_chunk_describe(b, hq, hk, d, s, lmax)
    assert text.startswith("attn_chunk "), text
    return {k: int(v) for k, v in re.findall(r"(rows|row_tiles|kv_tile|splits|chunk)=(\d+)", text)}


def lengths(g, s):
    """kv_len = S (one live split of many); chunk + 3 (at S = 16 the last live split lies wholly above the diagonal of the early rows:
    l = 0 there); an end mid-tile and mid-chunk; L_max."""
    assert g["splits"] >= 3 and g["chunk"] + 3 >= s
    return (s, g["chunk"] + 3, 2 * g["chunk"] + g["kv_tile"] // 2 + 1, LMAX)


@functools.lru_cache(maxsize=None)
def case(dtype, d, hq, hk, s, n, masked):
    """q as the [B, Hq, S, D] view of the [B, S, Hq, D] projection output, k, v, the bool mask (batch row 1 hides every key) and the
    float64 oracle with its bound -- computed once per case and left unchanged."""
    b = 3
    gen = torch.Generator().manual_seed(1000 * s + n + hq)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    q, k, v = r(b, s, hq, d).transpose(1, 2), r(b, hk, LMAX, d), r(b, hk, LMAX, d)
    mask = left_padded(b, s, n - s, LMAX, [min(7, n - s), LMAX, 0], "bool", dtype) if masked else None
    ref, pv = oracle(q, k, v, n, d ** -0.5, True, mask, weights=True)
    tol = bound(ref, pv, fp32_error(q, k, v, n, d ** -0.5, ref, True, mask), dtype)
    return q, k, v, mask, ref, tol


@pytest.mark.parametrize("on_device", (False, True), ids=("host_len", "device_len"))
@pytest.mark.parametrize("kind", (None, "bool", "additive"))
@pytest.mark.parametrize("hq,hk", GROUPS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_every_element_lies_within_the_bound(dtype, d, hq, hk, kind, on_device):
    for s in Q_LENS[(hq, hk)]:
        for n in lengths(geometry(3, hq, hk, d, s), s):
            q, k, v, mask, ref, tol = case(dtype, d, hq, hk, s, n, kind is not None)
            if kind == "additive":
                mask = torch.where(mask, torch.zeros((), dtype=dtype), torch.full((), torch.finfo(dtype).min, dtype=dtype))
            md = None if mask is None else mask.to(DEV)
            length = torch.tensor(n, dtype=torch.int64, device=DEV) if on_device else n
            got = ops.attn_chunk(q.to(DEV), k.to(DEV), v.to(DEV), length, mask=md).cpu()
            err = (got.double() - ref).abs()
            print(f"{tag(dtype)} d={d} ({hq},{hk}) S={s} n={n} {kind}: largest err / bound {(err / tol).max().item():.3f}")
            assert bool((err <= tol).all()), (s, n, (err / tol).max().item(), (err > tol).nonzero()[:4].tolist())
            if kind is not None:
                assert bool((got[1] == 0).all()), (s, n)          # the batch row whose mask hides every key


@pytest.mark.parametrize("hq,hk", GROUPS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_selection_is_bit_exact_and_repeats(dtype, d, hq, hk):
    """One key takes all the weight: out == V[pi(i)] exactly, so a wrong row packing or key permutation moves a row of V.  The same bits
    on a second call and with the partials region of the workspace full of NaN; the counters read zero afterwards."""
    b = 2
    for s in Q_LENS[(hq, hk)]:
        g = geometry(b, hq, hk, d, s)
        for n in lengths(g, s):
            q, k, v, pi, scaling = selection(b, hq, hk, d, s, n - s, dtype, lmax=LMAX)
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
            got = ops.attn_chunk(qd, kd, vd, n, scaling=scaling)
            want = selection_expected(v, pi, hk)
            wrong = (got.cpu().view(torch.int16) != want.view(torch.int16)).any(dim=-1)
            assert not bool(wrong.any()), (s, n, "first wrong (b, i, h)", wrong.nonzero()[:4].tolist())
            assert same(got, ops.attn_chunk(qd, kd, vd, n, scaling=scaling)), (s, n)
            nbytes = ops._lib.load().qllm_attn_chunk_workspace_bytes(b, hq, hk, d, s, LMAX)
            ws = ops.workspace(torch.device(DEV), nbytes)
            ws[COUNTER_BYTES:nbytes].view(torch.float32).fill_(float("nan"))
            assert same(got, ops.attn_chunk(qd, kd, vd, n, scaling=scaling)), (s, n)
            assert not bool(ws[:COUNTER_BYTES].any()), (s, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_one_captured_launch_serves_lengths_on_both_sides_of_a_chunk_boundary(dtype):
    d, hq, hk, s = 128, 8, 2, 9
    g = geometry(3, hq, hk, d, s)
    q, k, v, mask, _, _ = case(dtype, d, hq, hk, s, LMAX, True)
    qd, kd, vd, md = q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV)
    length = torch.tensor(LMAX, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, s, hq, d, dtype=dtype, device=DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_chunk(qd, kd, vd, length, mask=md, out=out)      # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_chunk(qd, kd, vd, length, mask=md, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for at in (g["chunk"], g["chunk"] + 1, s, 3 * g["chunk"] - 1, LMAX, g["chunk"] + 1):
        length.fill_(at)
        out.fill_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, ops.attn_chunk(qd, kd, vd, at, mask=md)), at


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_not_causal(dtype):
    d, hq, hk, s = 64, 8, 2, 9
    n = lengths(geometry(3, hq, hk, d, s), s)[2]
    q, k, v, _, _, _ = case(dtype, d, hq, hk, s, n, False)
    ref, pv = oracle(q, k, v, n, d ** -0.5, False, None, weights=True)
    tol = bound(ref, pv, fp32_error(q, k, v, n, d ** -0.5, ref, False, None), dtype)
    got = ops.attn_chunk(q.to(DEV), k.to(DEV), v.to(DEV), n, causal=False).cpu()
    assert bool(((got.double() - ref).abs() <= tol).all())
