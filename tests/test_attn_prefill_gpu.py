"""-m gpu: ops.attn_prefill (qllm_attn_prefill, csrc/attn_prefill.hip) on the device, fp16 and bf16, head_dim 64 and 128.

1. Selection, bit-exact: out[b, i, h, :] == V[pi(i)] for inputs on which one key takes all the weight (tests/attn_prefill_cases.py,
   `selection`; premises in tests/test_attn_prefill_inputs_cpu.py).  Any row / column swap, a wrong k order of the accumulator used as
   the next MFMA's operand, or a wrong transposed V read moves a row of V somewhere else.
2. Uniform: q = 0, so every visible key weighs 1 / count exactly: out is the mean of the integer V rows the row sees, within 1 ulp of the
   type (the division and the store are two roundings).  Counts exactly the keys the causal edge, the masks and the tile edges admit.
3. Random values against the float64 oracle, per element: `bound` (half an ulp at the oracle + 2 u sum p |v| + 8 e32; derived in
   attn_prefill_cases.py, not tuned).
4. Layouts and edges: views, strides, device lengths and their clamp, NaN behind the length, guard bands, repeatability, hipGraph replay.
5. Accuracy against the eager arithmetic in the type: E(kernel) <= M * E(eager), both against float64; M and the ratios of one run are in
   profiles/attn_prefill.md.

Sizes follow qllm_attn_prefill_describe (q_tile, kv_tile); the largest case is 2 q_tile + 1 rows behind kv_tile + 3 cached keys."""
import functools

import pytest
import torch

from attn_decode_cases import FAMILIES
from attn_prefill_cases import (DIMS, DTYPES, GROUPS, as_mask, bound, eager, fp32_error, left_padded, oracle, selection, selection_expected, tiles, ulp,
                                uniform, uniform_expected, visibility)
from gpu_util import guarded

from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M_EAGER = 1.8     # E(kernel) <= M_EAGER * E(eager): twice the largest ratio of profiles/attn_prefill.md ("Accuracy"), rounded up to one decimal


def tag(dtype):
    return str(dtype)[6:]


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev_len(n):
    return torch.tensor(n, dtype=torch.int64, device=DEV)


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


types = pytest.mark.parametrize("dtype", DTYPES, ids=tag)
dims = pytest.mark.parametrize("d", DIMS)


# ---- 1. selection ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", (1, 3))
@pytest.mark.parametrize("hq,hk", GROUPS)
@dims
@types
def test_selection_is_bit_exact(dtype, d, hq, hk, b):
    qt, kt = tiles(b, hq, hk, d)
    for s in (2, 3, qt - 1, qt, qt + 1, 2 * qt + 1):
        for q_start in (0, 1, kt - 1, kt, kt + 3):
            q, k, v, pi, scaling = selection(b, hq, hk, d, s, q_start, dtype)
            assert int(pi.max()) < q_start + s and bool((pi <= q_start + torch.arange(s)).all()) and (s < 8 or bool((pi[..., 1:] < pi[..., :-1]).any()))
            got = ops.attn_prefill(*dev(q, k, v), q_start + s, scaling=scaling).cpu()
            want = selection_expected(v, pi, hk)
            wrong = (bits(got) != bits(want)).any(dim=-1)
            assert not bool(wrong.any()), (s, q_start, "first wrong (b, i, h)", wrong.nonzero()[:4].tolist(), got[wrong][:1, :8], want[wrong][:1, :8])


# ---- 2. uniform --------------------------------------------------------------------------------------------------------------------------------
def uniform_masks(b, s, n, lwidth, kt, dtype):
    """name -> (mask or None as [B, 1, S, lwidth] bool, causal)."""
    q_start = n - s
    j, i = torch.arange(lwidth)[None, None, :], torch.arange(s)[None, :, None]
    causal = (j <= q_start + i).expand(b, s, lwidth)
    pads = [(3 * x + 2) % max(1, min(n - 1, kt + 5)) for x in range(b)]
    holes = causal & ((j * 7 + i * 3) % 5 != 0)
    tile_hidden = causal & ~((j >= kt) & (j < 2 * kt))                    # the second kv tile wholly hidden
    dead = causal.clone()
    dead[:, s // 2] = False                                              # a row with no visible key
    dead[-1, 0] = False
    free = ((j * 5 + i) % 3 != 0).expand(b, s, lwidth)                    # causal = 0: keys above the diagonal too
    return {"causal": (None, True), "not causal": (None, False), "left padding": (left_padded(b, s, q_start, lwidth, pads, "bool", dtype)[:, 0], True),
            "holes": (holes, True), "hidden tile": (tile_hidden, True), "dead rows": (dead, True), "free mask": (free, False)}


@pytest.mark.parametrize("hq,hk", ((8, 2), (7, 1)))
@dims
@types
def test_uniform_weights_count_exactly_the_visible_keys(dtype, d, hq, hk):
    b = 2
    qt, kt = tiles(b, hq, hk, d)
    for s, q_start in ((qt + 1, 2 * kt + 3), (3, kt), (2 * qt + 1, 0), (qt - 1, kt - 1)):
        n = q_start + s
        lwidth = n + 6
        q, k, v = uniform(b, hq, hk, d, s, n, dtype, lmax=lwidth)
        qd, kd, vd = dev(q, k, v)
        for name, (vis_mask, causal) in uniform_masks(b, s, n, lwidth, kt, dtype).items():
            outs = []
            for kind in ("bool", "additive") if vis_mask is not None else (None,):
                mask = None if kind is None else as_mask(vis_mask[:, None], kind, dtype)
                vis, _ = visibility(b, s, n, causal, mask)
                want, cnt = uniform_expected(v, vis, hq)
                if name == "dead rows":
                    assert int((cnt == 0).sum()) >= b
                if name == "hidden tile" and n > 2 * kt:
                    assert not bool(vis[:, :, kt:2 * kt].any())
                got = ops.attn_prefill(qd, kd, vd, n, mask=None if mask is None else mask.to(DEV), causal=causal).cpu()
                err = (got.double() - want).abs()
                assert bool((err <= ulp(want, dtype)).all()), (name, kind, s, q_start, (err / ulp(want, dtype)).max().item())
                assert bool((got[cnt == 0] == 0).all())
                outs.append(got)
            assert len(outs) == 1 or same(outs[0], outs[1]), (name, s, q_start)       # a zero byte and finfo.min hide alike: the same bits


# ---- 3. random values, per-element bound, and 5. the eager yardstick -----------------------------------------------------------------------
def normal(b, hq, hk, d, L, dtype, gen):
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    return r(b, hq, d), r(b, hk, L, d), r(b, hk, L, d), d ** -0.5


RANDOM = {"normal": normal, "peaked": FAMILIES["peaked"], "large_v": FAMILIES["large_v"]}


@functools.lru_cache(maxsize=None)
def random_case(name, hq, hk, d, dtype, s, n, masked):
    """q [1, Hq, S, D], k, v, scaling, mask, and the float64 oracle, sum p |v|, e32 and E(eager) -- computed once per case."""
    gen = torch.Generator().manual_seed(100 * s + n + hq)
    q, k, v, scaling = RANDOM[name](1, hq * s, hk, d, n + 5, dtype, gen)        # the families draw one row per head: S rows for each
    q = q.reshape(1, hq, s, d)
    mask = left_padded(1, s, n - s, n + 5, [min(7, n - s)], "bool", dtype) if masked else None
    ref, pv = oracle(q, k, v, n, scaling, True, mask, weights=True)
    e32 = fp32_error(q, k, v, n, scaling, ref, True, mask)
    e_eager = (eager(q, k, v, n, scaling, True, mask).double() - ref).abs().max().item()
    return q, k, v, scaling, mask, ref, pv, e32, e_eager


def random_cases():
    for d in DIMS:
        qt, kt = tiles(d=d)
        for hq, hk in ((8, 2), (5, 1), (8, 1)):
            for s, q_start, masked in ((2 * qt + 1, 3, False), (qt + 1, kt + 3, True), (5, 3 * kt - 2, False)):
                yield d, hq, hk, s, q_start + s, masked


@pytest.mark.parametrize("name", sorted(RANDOM))
@types
def test_random_values_within_the_derived_bound_and_the_eager_yardstick(dtype, name):
    worst, worst_ratio = 0.0, 0.0
    for d, hq, hk, s, n, masked in random_cases():
        q, k, v, scaling, mask, ref, pv, e32, e_eager = random_case(name, hq, hk, d, dtype, s, n, masked)
        got = ops.attn_prefill(*dev(q, k, v), n, mask=None if mask is None else mask.to(DEV), scaling=scaling).cpu()
        err, lim = (got.double() - ref).abs(), bound(ref, pv, e32, dtype)
        frac, ratio = (err / lim).max().item(), err.max().item() / e_eager
        print(f"{name} {tag(dtype)} d={d} {hq}x{hk} S={s} kv_len={n} masked={masked}: e_kernel {err.max().item():.3e} e32 {e32:.3e} e_eager {e_eager:.3e} "
              f"of the bound {frac:.3f} kernel/eager {ratio:.3f}")
        assert bool(torch.isfinite(got).all()) and frac <= 1.0, (name, d, hq, hk, s, n, err.max().item(), e32, frac)
        worst, worst_ratio = max(worst, frac), max(worst_ratio, ratio)
    print(f"{name} {tag(dtype)}: largest share of the bound {worst:.3f}, largest E(kernel) / E(eager) {worst_ratio:.3f} (M = {M_EAGER})")
    assert M_EAGER <= 2.0 and worst_ratio <= M_EAGER, (worst_ratio, M_EAGER)


# ---- 4. layouts and edges --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(dtype, d, hq=8, hk=2, b=2):
    qt, kt = tiles(b, hq, hk, d)
    s, n = qt + 3, qt + 3 + kt + 5
    lmax = n + kt + 9
    gen = torch.Generator().manual_seed(d + hq)
    r = lambda *shape: torch.randn(shape, generator=gen).to(dtype)
    q, k, v = r(b, hq, s, d), r(b, hk, lmax, d), r(b, hk, lmax, d)
    mask = left_padded(b, s, n - s, lmax, [0, 5], "bool", dtype)
    qd, kd, vd, md = dev(q, k, v, mask)
    return dict(s=s, n=n, lmax=lmax, q=q, k=k, v=v, mask=mask, qd=qd, kd=kd, vd=vd, md=md, plain=ops.attn_prefill(qd, kd, vd, n),
                masked=ops.attn_prefill(qd, kd, vd, n, mask=md), b=b, hq=hq, hk=hk, kt=kt)


@dims
@types
def test_views_strides_and_mask_layouts_give_the_same_bits(dtype, d):
    c = edge_case(dtype, d)
    b, hq, hk, s, lmax, n = c["b"], c["hq"], c["hk"], c["s"], c["lmax"], c["n"]
    ref64 = oracle(c["q"], c["k"], c["v"], n, d ** -0.5)
    assert (c["plain"].cpu().double() - ref64).abs().max() < 0.05                                       # the reference of this test is itself attention
    # q: the projection output [B, S, Hq, D] viewed as [B, Hq, S, D], and that inside a wider q/k/v buffer
    q_t = c["qd"].transpose(1, 2).contiguous().transpose(1, 2)
    wide = torch.full((b, s, (hq + 2 * hk) * d), float("nan"), dtype=dtype, device=DEV)
    wide[..., :hq * d] = c["qd"].transpose(1, 2).reshape(b, s, hq * d)
    q_w = wide[..., :hq * d].view(b, s, hq, d).transpose(1, 2)
    assert ops.attn_prefill_plan(q_t, c["kd"], c["vd"], n)[6:9] == (s * hq * d, d, hq * d) and ops.attn_prefill_plan(q_w, c["kd"], c["vd"], n)[8] == (hq + 2 * hk) * d
    assert same(ops.attn_prefill(q_t, c["kd"], c["vd"], n), c["plain"]) and same(ops.attn_prefill(q_w, c["kd"], c["vd"], n), c["plain"])
    # caches in [B, L, Hkv, D] memory, and as a slice of longer caches
    k_t, v_t = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (c["kd"], c["vd"]))
    assert ops.attn_prefill_plan(c["qd"], k_t, v_t, n)[9:12] == (lmax * hk * d, d, hk * d)
    assert same(ops.attn_prefill(c["qd"], k_t, v_t, n), c["plain"])
    big_k, big_v = (torch.full((b, hk, lmax + 24, d), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
    big_k[:, :, 8:8 + lmax], big_v[:, :, 8:8 + lmax] = c["kd"], c["vd"]
    assert same(ops.attn_prefill(c["qd"], big_k[:, :, 8:8 + lmax], big_v[:, :, 8:8 + lmax], n, mask=c["md"]), c["masked"])
    # masks: batch stride 0 (one mask for the batch, expanded), a 3-D mask, a mask inside a wider buffer, the additive form
    one = c["md"][:1].expand(b, 1, s, lmax)
    assert ops.attn_prefill_plan(c["qd"], c["kd"], c["vd"], n, mask=one)[13:] == (lmax, 0, lmax)
    assert same(ops.attn_prefill(c["qd"][:1], c["kd"][:1], c["vd"][:1], n, mask=c["md"][:1]), ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, mask=one)[:1])
    assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, mask=c["md"][:, 0]), c["masked"])
    mwide = torch.zeros(b, 1, s, lmax + 37, dtype=torch.bool, device=DEV)
    mwide[..., 3:3 + lmax] = c["md"]
    assert ops.attn_prefill_plan(c["qd"], c["kd"], c["vd"], n, mask=mwide[..., 3:3 + lmax])[13:] == (lmax, s * (lmax + 37), lmax + 37)
    assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, mask=mwide[..., 3:3 + lmax]), c["masked"])
    assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, mask=as_mask(c["mask"], "additive", dtype).to(DEV)), c["masked"])
    assert not same(c["masked"], c["plain"])
    # the same bits on two calls, and into a given `out`
    out = torch.empty_like(c["plain"])
    assert ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, out=out) is out and same(out, c["plain"]) and same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], n, mask=c["md"]), c["masked"])


@dims
@types
def test_device_lengths_the_clamp_and_nan_behind_the_length(dtype, d):
    c = edge_case(dtype, d)
    s, lmax, n = c["s"], c["lmax"], c["n"]
    assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], dev_len(n)), c["plain"])
    assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], dev_len(n), mask=c["md"]), c["masked"])
    # a device length below q_len counts as q_len, one above max_len as max_len
    for given, counted in ((0, s), (-7, s), (s - 1, s), (lmax + 1, lmax), (1 << 40, lmax)):
        assert same(ops.attn_prefill(c["qd"], c["kd"], c["vd"], dev_len(given)), ops.attn_prefill(c["qd"], c["kd"], c["vd"], counted)), given
    # NaN in every cache position >= kv_len: the bits of zeros there
    for length in (n, s, c["kt"] * ((n + c["kt"] - 1) // c["kt"])):
        kz, vz, kn, vn = c["kd"].clone(), c["vd"].clone(), c["kd"].clone(), c["vd"].clone()
        kz[:, :, length:], vz[:, :, length:], kn[:, :, length:], vn[:, :, length:] = 0, 0, float("nan"), float("nan")
        for mask in (None, c["md"]):
            got = ops.attn_prefill(c["qd"], kn, vn, length, mask=mask)
            assert bool(torch.isfinite(got).all()) and same(got, ops.attn_prefill(c["qd"], kz, vz, length, mask=mask)), length
            assert same(got, ops.attn_prefill(c["qd"], kn, vn, dev_len(length), mask=mask))


@dims
@types
def test_nothing_outside_out_is_written_and_the_caches_are_only_read(dtype, d):
    c = edge_case(dtype, d)
    n = c["n"]
    (kbuf, kv), (vbuf, vv), (qbuf, qv) = guarded(c["kd"]), guarded(c["vd"]), guarded(c["qd"])
    obuf, ov = guarded(torch.zeros_like(c["plain"]))
    before = [bits(t).clone() for t in (kbuf, vbuf, qbuf, obuf)]
    for mask, want in ((None, c["plain"]), (c["md"], c["masked"])):
        ops.attn_prefill(qv, kv, vv, n, mask=mask, out=ov)
        assert same(ov, want)                                               # no NaN of a guard band was read into the result
    torch.cuda.synchronize()
    lead = (obuf.numel() - ov.numel()) // 2
    assert torch.equal(bits(kbuf), before[0]) and torch.equal(bits(vbuf), before[1]) and torch.equal(bits(qbuf), before[2])
    assert torch.equal(bits(obuf)[:lead], before[3][:lead]) and torch.equal(bits(obuf)[lead + ov.numel():], before[3][lead + ov.numel():])


@pytest.mark.parametrize("d", (128,))
@types
def test_one_captured_launch_serves_two_lengths(dtype, d):
    """Captured with the process's default queue settings; the length is read from device memory at replay."""
    c = edge_case(dtype, d)
    s, lmax, n = c["s"], c["lmax"], c["n"]
    length = dev_len(n)
    out = torch.empty_like(c["plain"])
    ops.attn_prefill(c["qd"], c["kd"], c["vd"], length, mask=c["md"], out=out)          # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attn_prefill(c["qd"], c["kd"], c["vd"], length, mask=c["md"], out=out)
    for at in (s + 1, n, lmax):
        length.fill_(at)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, ops.attn_prefill(c["qd"], c["kd"], c["vd"], at, mask=c["md"])), at
