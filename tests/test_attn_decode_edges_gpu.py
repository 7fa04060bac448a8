"""-m gpu: the parts of csrc/attn_decode.hip that tests/test_attn_decode_gpu.py's case matrix never launches -- every group size 1..8 and
both combine layouts with full runs of splits, caches that are not contiguous, masks other than a hidden prefix, the length's edges, value
ranges on which the online softmax rescales, guard bands around every operand with a dirty workspace, and the counter page shared with
the split-K linears.

Tolerance (tests/attn_decode_cases.py, `bound`): per element, half the spacing of the output type at the float64 oracle -- the kernel
rounds once, from fp32 -- plus 8 times e32, the largest error of the op restated in fp32 on the CPU against the same oracle, of the same
case.  Neither term is measured on the kernel.  tests/test_attn_decode_inputs_cpu.py proves the inputs' premises (finite, not
one-key-wins, rising / falling tile maxima, the reference inside the bound with factor 1).  Every accuracy check prints e_kernel, e32, the
largest bound and the largest e_kernel / bound of its case (pytest -s); profiles/attn_decode.md holds the figures of one run."""
import functools

import pytest
import torch

from attn_decode_cases import (BATCHES, DIMS, DTYPES, FAMILIES, FAMILY_HEADS, bound, eager, family_inputs, family_lengths, fp32_error, geometry,
                               mid_split, oracle, parse_describe, reduced_lengths)
from gpu_util import guarded, randx, synth, to_layer

from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTERS = 16384


def tag(dtype):
    return str(dtype)[6:]


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def counters_clean():
    return int(ops.workspace(torch.device(DEV), 0)[:COUNTERS].count_nonzero()) == 0


def dev_len(n):
    return torch.tensor(n, dtype=torch.int64, device=DEV)


def randn(shape, dtype, gen):
    return torch.randn(shape, generator=gen).to(dtype)


def held(got, ref, e32, dtype, what):
    """Prints the case's figures and holds the kernel's result (CPU tensor) to `bound`, element by element; returns e_kernel."""
    err, lim = (got.double() - ref).abs(), bound(ref, e32, dtype)
    ratio = (err / lim).max().item()
    print(f"{what}: e_kernel {err.max().item():.3e} e32 {e32:.3e} bound {lim.max().item():.3e} ratio {ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, err.max().item(), e32, ratio)
    return err.max().item()


@functools.lru_cache(maxsize=4)
def normal_inputs(b, hq, hk, d, dtype, lmax, seed):
    """N(0, 1) q, k, v and one new row, on the CPU and on the device (shared by the tests of a case; nobody writes to them)"""
    gen = torch.Generator().manual_seed(seed)
    c = {"q": randn((b, hq, d), dtype, gen), "k": randn((b, hk, lmax, d), dtype, gen), "v": randn((b, hk, lmax, d), dtype, gen),
         "kn": randn((b, hk, d), dtype, gen), "vn": randn((b, hk, d), dtype, gen)}
    c.update({"qd": c["q"][:, :, None].to(DEV), "kd": c["k"].to(DEV), "vd": c["v"].to(DEV), "knd": c["kn"][:, :, None].to(DEV), "vnd": c["vn"][:, :, None].to(DEV)})
    return c


# ---- 1. every group size ----------------------------------------------------------------------------------------------------------------------
S32_LMAX = 2047     # 32 tiles of 64 at head_dim 128: 32 splits of one tile where two blocks per compute unit allow that many, the last ragged
GROUP_CASES = ([(g * hk, hk, d, dt, False) for g in range(1, 9) for hk in (1, 2) for d in DIMS for dt in DTYPES]
               + [(g, 1, 128, dt, True) for g in (5, 6, 8) for dt in DTYPES])
GROUP_IDS = [f"{hq}x{hk}-d{d}-{tag(dt)}" + ("-splits32" if s32 else "") for hq, hk, d, dt, s32 in GROUP_CASES]
group_cases = pytest.mark.parametrize("hq,hk,d,dtype,s32", GROUP_CASES, ids=GROUP_IDS)


def group_geometry(hq, hk, d, s32):
    """(L_max, geometry, lengths) at batch 1.  s32: the launch whose R = 2 combine (G * D / 8 > 64) folds two runs of 16 splits, each two
    full loads of kCombine = 8; the premise is the split count the library states."""
    if not s32:
        lmax, geo = geometry(1, hq, hk, d)
    else:
        lmax, geo = S32_LMAX, parse_describe(ops.attn_decode_describe(1, hq, hk, d, S32_LMAX))
        if geo["splits"] < 17:
            pytest.skip(f"{geo['splits']} splits at L_max {lmax}: too few compute units for a run of more than 8 splits")
        assert geo["splits"] == 32 and geo["chunk"] == geo["tile"] == 64 and hq * d // 8 > 64, geo
    assert geo["group"] == hq // hk
    return lmax, geo, reduced_lengths(lmax, geo)


@group_cases
def test_group_sizes_one_key_wins_bit_for_bit(hq, hk, d, dtype, s32):
    """test_attn_decode_gpu.py's construction at batch 1: q = 16 e_g plus +-1 noise in columns 8..23, K +-1 noise there and 16 in column g
    of the winner's position, scaling 0.25 -- the winner scores at least 60, every other at most 4, the output is the winner's V row.
    Every head wins once at every length of the list with all splits live; then kv_len = each length with the winner last and a key
    that would win behind it."""
    lmax, geo, ls = group_geometry(hq, hk, d, s32)
    grp = hq // hk
    gen = torch.Generator().manual_seed(hq * 131 + d)
    v = torch.randint(1, 9, (1, hk, lmax, d), generator=gen).float() * (torch.randint(0, 2, (1, hk, lmax, d), generator=gen) * 2 - 1)
    k = torch.zeros(1, hk, lmax, d)
    k[..., 8:24] = torch.randint(-1, 2, (1, hk, lmax, 16), generator=gen).float()
    q = torch.zeros(1, hq, d)
    q[..., 8:24] = torch.randint(-1, 2, (1, hq, 16), generator=gen).float()
    noise = torch.einsum("bkgd,bknd->bkgn", q.view(1, hk, grp, d), k) * 0.25
    assert 64 - 2 * noise.abs().max().item() >= 40
    hi = torch.arange(hq)
    q[0, hi, hi % grp] = 16.0
    qd, kd, vd = q.to(dtype)[:, :, None].to(DEV), k.to(dtype).to(DEV), v.to(dtype).to(DEV)
    v, at, hi_d = v.to(dtype), torch.tensor(ls), hi.to(DEV)
    for r in range(len(ls)):
        pos = at[(hi + r) % len(ls)] - 1
        k1 = kd.clone()
        k1[0, hi_d // grp, pos.to(DEV), hi_d % grp] = 16.0
        got = ops.attn_decode(qd, k1, vd, lmax, scaling=0.25).cpu()
        assert same(got[0], v[0, hi // grp, pos]), r
    for n in ls:
        k1, v1 = kd.clone(), vd.clone()
        k1[:, :, n - 1:, :grp] = 16.0
        v1[:, :, n:] = 64.0
        got = ops.attn_decode(qd, k1, v1, n, scaling=0.25).cpu()
        assert same(got[0], v[0, hi // grp, n - 1]), n


@group_cases
def test_group_sizes_uniform_weights_exact_mean(hq, hk, d, dtype, s32):
    """q = 0 and integer V in pairs (x, -x) from position 16 on: the mean over a power-of-two length is representable, and so is the mean
    over every length of the list that is one."""
    lmax, geo, ls = group_geometry(hq, hk, d, s32)
    gen = torch.Generator().manual_seed(hq + d)
    v = torch.randint(-8, 9, (1, hk, lmax, d), generator=gen).float()
    v[:, :, 17:lmax:2] = -v[:, :, 16:lmax - 1:2]
    kd, vd = randn((1, hk, lmax, d), dtype, gen).to(DEV), v.to(dtype).to(DEV)
    qd = torch.zeros(1, hq, 1, d, dtype=dtype, device=DEV)
    n = 1
    while n <= lmax:
        mean = v[:, :, :n].double().mean(dim=2)
        want = mean.to(dtype)
        assert torch.equal(want.double(), mean)
        got = ops.attn_decode(qd, kd, vd, n).cpu()
        assert torch.equal(got, want.repeat_interleave(hq // hk, dim=1)), n
        n *= 2


@group_cases
def test_group_sizes_accuracy(hq, hk, d, dtype, s32):
    """N(0, 1) values, scaling D^-1/2: no worse than the eager arithmetic, as the old matrix asks, and inside `bound`."""
    lmax, geo, ls = group_geometry(hq, hk, d, s32)
    c = normal_inputs(1, hq, hk, d, dtype, lmax, 7 * hq + d)
    bad = []
    for n in ls:
        ref = oracle(c["q"], c["k"], c["v"], n, d ** -0.5)
        e32, _ = fp32_error(c["q"], c["k"], c["v"], n, d ** -0.5, ref)
        got = ops.attn_decode(c["qd"], c["kd"], c["vd"], n).cpu()
        e_kernel = held(got, ref, e32, dtype, f"groups {hq}x{hk} d={d} {tag(dtype)} kv_len={n}")
        e_eager = (eager(c["q"], c["k"], c["v"], n, d ** -0.5).double() - ref).abs().max().item()
        if e_kernel > e_eager:
            bad.append((n, e_kernel, e_eager))
    assert not bad, bad


# ---- 2. cache layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(hq, hk, d, b, dt) for (hq, hk) in ((8, 2), (6, 1)) for d in DIMS for b in BATCHES for dt in DTYPES]
LAYOUT_IDS = [f"{hq}x{hk}-d{d}-b{b}-{tag(dt)}" for hq, hk, d, b, dt in LAYOUT_CASES]
layout_cases = pytest.mark.parametrize("hq,hk,d,b,dtype", LAYOUT_CASES, ids=LAYOUT_IDS)


def run_layout(hq, hk, d, b, dtype, new_buffer, view, strides=None):
    """Every (append, host / device length, length) call on caches laid out by `new_buffer` (an uninitialised or NaN buffer) and `view`
    (the [B, Hkv, L, D] cache inside a buffer) against the same call on contiguous caches: the same output bits, and afterwards the
    WHOLE buffers hold what they held -- bit for bit, the NaN around the view included -- but for the view, which holds the contiguous
    cache (so with an append the new row, at its place, and nothing else)."""
    lmax, geo = geometry(b, hq, hk, d)
    c = normal_inputs(b, hq, hk, d, dtype, lmax, 19)
    for append in (False, True):
        for on_device in (False, True):
            for n in (mid_split(geo) * geo["chunk"], lmax - 1):
                kc, vc = c["kd"].clone(), c["vd"].clone()
                kb, vb = new_buffer(lmax), new_buffer(lmax)
                view(kb).copy_(kc), view(vb).copy_(vc)
                k_want, v_want = kb.clone(), vb.clone()
                if strides is not None:
                    assert ops.attn_decode_plan(c["qd"], view(kb), view(vb), n)[11:14] == strides(lmax), (ops.attn_decode_plan(c["qd"], view(kb), view(vb), n), strides(lmax))
                new = (c["knd"], c["vnd"]) if append else ()
                want = ops.attn_decode(c["qd"], kc, vc, dev_len(n) if on_device else n, *new)
                got = ops.attn_decode(c["qd"], view(kb), view(vb), dev_len(n) if on_device else n, *new)
                what = (append, on_device, n)
                assert same(got, want), what
                if append:
                    assert same(kc[:, :, n], c["knd"][:, :, 0]) and same(vc[:, :, n], c["vnd"][:, :, 0]), what
                view(k_want).copy_(kc), view(v_want).copy_(vc)
                assert same(kb, k_want) and same(vb, v_want), what


@layout_cases
def test_cache_in_batch_position_head_memory(hq, hk, d, b, dtype):
    """[B, L, Hkv, D] memory viewed as [B, Hkv, L, D]: the position stride is Hkv * D, the head stride D."""
    run_layout(hq, hk, d, b, dtype, lambda L: torch.full((b, L, hk, d), float("nan"), dtype=dtype, device=DEV), lambda t: t.permute(0, 2, 1, 3),
               lambda L: (L * hk * d if b > 1 else 0, d if hk > 1 else 0, hk * d))


@layout_cases
def test_cache_as_a_slice_of_a_larger_one(hq, hk, d, b, dtype):
    """big[1:1+B, 1:1+Hkv, 8:8+L] of a NaN-filled cache: every element of `big` outside the slice is bit-unchanged."""
    run_layout(hq, hk, d, b, dtype, lambda L: torch.full((b + 2, hk + 2, L + 16, d), float("nan"), dtype=dtype, device=DEV),
               lambda t: t[1:1 + b, 1:1 + hk, 8:8 + t.shape[2] - 16],
               lambda L: ((hk + 2) * (L + 16) * d if b > 1 else 0, (L + 16) * d if hk > 1 else 0, d))


@pytest.mark.parametrize("hq,d,dtype", [(6, d, dt) for d in DIMS for dt in DTYPES], ids=[f"6x1-d{d}-b1-{tag(dt)}" for d in DIMS for dt in DTYPES])
def test_cache_extents_of_one_with_odd_strides(hq, d, dtype):
    """B = 1 and Hkv = 1 with nominal strides 7 and 13 (as_strided): a stride counts as 0 where the extent is 1, and the call is served."""
    run_layout(hq, 1, d, 1, dtype, lambda L: torch.full((L * d + 64,), float("nan"), dtype=dtype, device=DEV),
               lambda t: torch.as_strided(t, (1, 1, (t.numel() - 64) // d, d), (7, 13, d, 1), 8), lambda L: (0, 0, d))


@layout_cases
def test_caches_of_two_layouts_are_refused_before_any_launch(hq, hk, d, b, dtype):
    lmax, geo = geometry(b, hq, hk, d)
    c = normal_inputs(b, hq, hk, d, dtype, lmax, 19)
    other = torch.empty(b, lmax, hk, d, dtype=dtype, device=DEV).permute(0, 2, 1, 3)
    other.copy_(c["vd"])
    for k, v in ((c["kd"], other), (other, c["vd"])):
        for new in ((), (c["knd"], c["vnd"])):
            out = torch.full((b, hq, d), 7.0, dtype=dtype, device=DEV)
            with pytest.raises(ops.QllmUnsupported):
                ops.attn_decode(c["qd"], k, v, lmax - 1, *new, out=out)
            assert bool((out == 7.0).all())
    assert same(other, c["vd"])


# ---- 3. masks ---------------------------------------------------------------------------------------------------------------------------------
MASK_CASES = [(hq, hk, d, dt) for (hq, hk) in ((4, 4), (28, 4)) for d in DIMS for dt in DTYPES]
MASK_IDS = [f"{hq}x{hk}-d{d}-b3-{tag(dt)}" for hq, hk, d, dt in MASK_CASES]
mask_cases = pytest.mark.parametrize("hq,hk,d,dtype", MASK_CASES, ids=MASK_IDS)
MB = 3


def mask_setup(hq, hk, d, dtype):
    """batch 3; kv_len = L_max - 1: every split live, the last ragged.  Every mask is L_max long, so it also serves a length on the device."""
    lmax, geo = geometry(MB, hq, hk, d)
    return lmax, geo, lmax - 1, normal_inputs(MB, hq, hk, d, dtype, lmax, 23)


def both_lengths(c, n, mask):
    """The call with the length on the host and on the device: the same bits; on the CPU."""
    m4 = mask.to(DEV)[:, None, None, :] if mask.dim() == 2 else mask.to(DEV)
    a = ops.attn_decode(c["qd"], c["kd"], c["vd"], n, mask=m4)
    e = ops.attn_decode(c["qd"], c["kd"], c["vd"], dev_len(n), mask=m4)
    assert same(a, e)
    return a.cpu()


def additive_of(visible, dtype, hidden):
    return torch.zeros(visible.shape, dtype=dtype).masked_fill(~visible, hidden)


def patterns(lmax, geo, n):
    """name -> visible [3, L_max] bool.  holes: every third key hidden, from another phase per batch entry; middle: a whole split of the
    middle hidden (two of them for the second entry where there are five), so the combine folds a (kNoMax, 0, 0) partial between live ones;
    last: only key n - 1 visible."""
    pos, c, mid = torch.arange(lmax), geo["chunk"], mid_split(geo)
    holes = torch.stack([(pos + i) % 3 != 0 for i in range(MB)])
    middle = torch.ones(MB, lmax, dtype=torch.bool)
    middle[:, mid * c:(mid + 1) * c] = False
    if geo["splits"] >= 5:
        middle[1, (mid - 1) * c:mid * c] = False
    assert mid >= 1 and (mid + 1) * c < n
    last = torch.zeros(MB, lmax, dtype=torch.bool)
    last[:, n - 1] = True
    return {"holes": holes, "middle": middle, "last": last}


@mask_cases
def test_finite_biases(hq, hk, d, dtype):
    """-m (n - 1 - pos), m = 1/16 and 1/2, rounded to the type (the oracle adds the rounded values), the steeper for the later batch entry:
    nothing is hidden, every key's weight is scaled."""
    lmax, geo, n, c = mask_setup(hq, hk, d, dtype)
    for m in (1 / 16, 1 / 2):
        bias = torch.stack([-(m * (1 + i / 4)) * (n - 1 - torch.arange(lmax, dtype=torch.float64)) for i in range(MB)]).to(dtype)
        got = both_lengths(c, n, bias)
        ref = oracle(c["q"], c["k"], c["v"], n, d ** -0.5, bias=bias)
        e32, _ = fp32_error(c["q"], c["k"], c["v"], n, d ** -0.5, ref, mask=bias[:, None, None, :])
        held(got, ref, e32, dtype, f"bias m={m} {hq}x{hk} d={d} {tag(dtype)} kv_len={n}")


@pytest.mark.parametrize("pattern", ("holes", "middle", "last"))
@mask_cases
def test_bool_lowest_and_minus_inf_hide_the_same_keys(hq, hk, d, dtype, pattern):
    """A bool mask, 0 / finfo.min and 0 / -inf: one result, bit for bit, inside `bound` of the oracle that hides the same keys."""
    lmax, geo, n, c = mask_setup(hq, hk, d, dtype)
    visible = patterns(lmax, geo, n)[pattern]
    got = both_lengths(c, n, visible)
    assert same(got, both_lengths(c, n, additive_of(visible, dtype, torch.finfo(dtype).min)))
    assert same(got, both_lengths(c, n, additive_of(visible, dtype, float("-inf"))))
    ref = oracle(c["q"], c["k"], c["v"], n, d ** -0.5, visible)
    e32, _ = fp32_error(c["q"], c["k"], c["v"], n, d ** -0.5, ref, mask=visible[:, None, None, :])
    held(got, ref, e32, dtype, f"mask {pattern} {hq}x{hk} d={d} {tag(dtype)} kv_len={n}")
    if pattern == "last":
        assert same(got, c["v"][:, :, n - 1].repeat_interleave(hq // hk, dim=1))


@mask_cases
def test_a_bias_with_holes_as_bool_times_bias_would_be(hq, hk, d, dtype):
    """A finite bias on the visible keys and -inf / finfo.min on every third: both spellings give the same bits, inside `bound`."""
    lmax, geo, n, c = mask_setup(hq, hk, d, dtype)
    visible = patterns(lmax, geo, n)["holes"]
    bias = (-(n - 1 - torch.arange(lmax, dtype=torch.float64)) / 16).to(dtype).expand(MB, lmax)
    got = both_lengths(c, n, bias.masked_fill(~visible, float("-inf")))
    assert same(got, both_lengths(c, n, bias.masked_fill(~visible, torch.finfo(dtype).min)))
    ref = oracle(c["q"], c["k"], c["v"], n, d ** -0.5, visible, bias)
    e32, _ = fp32_error(c["q"], c["k"], c["v"], n, d ** -0.5, ref, mask=bias.masked_fill(~visible, float("-inf"))[:, None, None, :])
    held(got, ref, e32, dtype, f"bias with holes {hq}x{hk} d={d} {tag(dtype)} kv_len={n}")


@mask_cases
def test_one_mask_row_for_the_batch(hq, hk, d, dtype):
    """[1, 1, 1, L] (mask_batch = 0) against the same row repeated per batch entry, bool and additive."""
    lmax, geo, n, c = mask_setup(hq, hk, d, dtype)
    visible = patterns(lmax, geo, n)["holes"][1:2]
    bias = (-(n - 1 - torch.arange(lmax, dtype=torch.float64)) / 16).to(dtype)[None].masked_fill(~visible, float("-inf"))
    for row in (visible, bias):
        assert ops.attn_decode_plan(c["qd"], c["kd"], c["vd"], n, mask=row.to(DEV)[:, None, None, :])[-2:] == (lmax, 0)
        assert same(both_lengths(c, n, row[:, None, None, :]), both_lengths(c, n, row.repeat(MB, 1)))


@mask_cases
def test_a_longer_mask_inside_a_wider_buffer(hq, hk, d, dtype):
    """[B, L + 40] as columns 33 .. of a [B, L + 104] buffer: the batch stride is neither L nor L + 40; NaN (additive) and True (bool, where
    False could only hide) outside the slice and behind L_max."""
    lmax, geo, n, c = mask_setup(hq, hk, d, dtype)
    visible = patterns(lmax, geo, n)["holes"]
    bias = (-(n - 1 - torch.arange(lmax, dtype=torch.float64)) / 16).to(dtype).expand(MB, lmax).masked_fill(~visible, float("-inf"))
    for row, outside in ((visible, True), (bias, float("nan"))):
        wide = torch.full((MB, lmax + 104), outside, dtype=row.dtype)
        wide[:, 33:33 + lmax] = row
        view = wide.to(DEV)[:, 33:33 + lmax + 40]
        assert ops.attn_decode_plan(c["qd"], c["kd"], c["vd"], dev_len(n), mask=view)[-2:] == (lmax + 40, lmax + 104)
        a = ops.attn_decode(c["qd"], c["kd"], c["vd"], n, mask=view)
        e = ops.attn_decode(c["qd"], c["kd"], c["vd"], dev_len(n), mask=view[:, None, None, :])
        assert same(a, e) and same(a.cpu(), both_lengths(c, n, row)) and bool(torch.isfinite(a).all())


def test_bf16_bias_below_the_floor_of_the_running_maximum_gives_zeros():
    """Documented in csrc/attn_decode.hip: the running maximum starts at -1e30, so a row whose visible keys ALL carry a finite bf16 bias
    below about -7e29 (above finfo.min, which hides) stores zeros, not the softmax among them.  fp16 has no such value.  Pinned here so
    that changing it is a decision; a bias of -1e29 on every key is an ordinary softmax."""
    hq, hk, d, dtype = 4, 4, 64, torch.bfloat16
    lmax, geo = geometry(1, hq, hk, d)
    c = normal_inputs(1, hq, hk, d, dtype, lmax, 29)
    n = lmax - 1
    low = torch.full((1, lmax), -1e30, dtype=dtype)
    assert torch.finfo(dtype).min < low[0, 0].item() < -7e29
    got = both_lengths(c, n, low)
    assert torch.equal(bits(got), torch.zeros_like(bits(got)))
    # fp32 scores of magnitude 1e29 have a spacing of about 1e22: the N(0, 1) part of every score is absorbed and the weights are uniform.
    # An fp32 sum of n terms in any order errs by at most n 2^-24 sum |v|, so the mean by at most n 2^-24 max |v|.
    shifted = both_lengths(c, n, torch.full((1, lmax), -1e29, dtype=dtype))
    held(shifted, c["v"][:, :, :n].double().mean(dim=2), n * 2.0 ** -24 * c["v"].abs().max().item() / 8, dtype, "bf16 bias -1e29")


# ---- 4. length edges --------------------------------------------------------------------------------------------------------------------------
@layout_cases
def test_no_key_at_all_stores_zeros(hq, hk, d, b, dtype):
    """kv_len = 0 without an append, host and device, without a mask and with a bool one: split 0 stores the zeros (over NaN), reads no
    cache row (all NaN) and takes no ticket."""
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(31)
    qd = randn((b, hq, 1, d), dtype, gen).to(DEV)
    kd = torch.full((b, hk, lmax, d), float("nan"), dtype=dtype, device=DEV)
    vd = kd.clone()
    for mask in (None, torch.ones(b, 1, 1, lmax, dtype=torch.bool, device=DEV)):
        for length in (0, dev_len(0), dev_len(-5)):
            out = torch.full((b, hq, d), float("nan"), dtype=dtype, device=DEV)
            assert ops.attn_decode(qd, kd, vd, length, mask=mask, out=out) is out
            assert torch.equal(bits(out), torch.zeros_like(bits(out))) and counters_clean()


@layout_cases
def test_a_device_length_outside_the_cache_is_clamped(hq, hk, d, b, dtype):
    """Without an append -5, L_max + 1 and 2^40 on the device are 0, L_max and L_max."""
    lmax, geo = geometry(b, hq, hk, d)
    c = normal_inputs(b, hq, hk, d, dtype, lmax, 19)
    none, full = ops.attn_decode(c["qd"], c["kd"], c["vd"], 0), ops.attn_decode(c["qd"], c["kd"], c["vd"], lmax)
    mask = torch.ones(b, lmax, dtype=torch.bool, device=DEV)
    for length, want in ((-5, none), (lmax + 1, full), (2 ** 40, full), (-2 ** 40, none)):
        assert same(ops.attn_decode(c["qd"], c["kd"], c["vd"], dev_len(length)), want), length
        assert same(ops.attn_decode(c["qd"], c["kd"], c["vd"], dev_len(length), mask=mask), want), length
        assert counters_clean()
    assert torch.equal(bits(none), torch.zeros_like(bits(none)))
    assert same(c["kd"], c["k"].to(DEV)) and same(c["vd"], c["v"].to(DEV))


def lengths_against_the_bound(c, b, hq, hk, d, dtype, lmax, ns, what):
    for n in ns:
        ref = oracle(c["q"], c["k"], c["v"], n, d ** -0.5)
        e32, _ = fp32_error(c["q"], c["k"], c["v"], n, d ** -0.5, ref)
        held(ops.attn_decode(c["qd"], c["kd"], c["vd"], n).cpu(), ref, e32, dtype, f"{what} {hq}x{hk} d={d} b={b} {tag(dtype)} kv_len={n}")
        assert counters_clean()
    n = ns[-2]                                   # one append: the new row lands at position n, n + 1 keys are attended
    k1, v1 = c["kd"].clone(), c["vd"].clone()
    k1[:, :, n], v1[:, :, n] = float("nan"), float("nan")
    got = ops.attn_decode(c["qd"], k1, v1, n, c["knd"], c["vnd"])
    k2, v2 = c["kd"].clone(), c["vd"].clone()
    k2[:, :, n], v2[:, :, n] = c["knd"][:, :, 0], c["vnd"][:, :, 0]
    assert same(k1, k2) and same(v1, v2) and same(got, ops.attn_decode(c["qd"], k2, v2, n + 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_one_split_over_many_tiles_and_a_deep_grid(dtype):
    """B = 65, 8 kv heads, head_dim 128, L_max = 200: with batch * kv_heads >= two blocks per compute unit there is ONE split, whose block
    loops over all four tiles and stores directly; gridDim.z = 65."""
    b, hq, hk, d, lmax = 65, 8, 8, 128, 200
    geo = parse_describe(ops.attn_decode_describe(b, hq, hk, d, lmax))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if b * hk < 2 * cus:
        pytest.skip(f"{cus} compute units: batch * kv_heads = {b * hk} is below two blocks per unit, the launch has {geo['splits']} splits")
    assert geo["splits"] == 1 and geo["chunk"] >= lmax > 3 * geo["tile"], geo
    lengths_against_the_bound(normal_inputs(b, hq, hk, d, dtype, lmax, 37), b, hq, hk, d, dtype, lmax, (1, 64, 65, 199, 200), "one split")


@pytest.mark.parametrize("hq,hk,d,dtype", [(8, 2, d, dt) for d in DIMS for dt in DTYPES], ids=[f"8x2-d{d}-{tag(dt)}" for d in DIMS for dt in DTYPES])
def test_a_cache_shorter_than_one_tile(hq, hk, d, dtype):
    lmax = 50
    geo = parse_describe(ops.attn_decode_describe(1, hq, hk, d, lmax))
    assert geo["splits"] == 1 and lmax <= geo["tile"] == geo["chunk"], geo
    lengths_against_the_bound(normal_inputs(1, hq, hk, d, dtype, lmax, 41), 1, hq, hk, d, dtype, lmax, (1, 2, 49, 50), "one tile")


# ---- 5. value families ------------------------------------------------------------------------------------------------------------------------
FAMILY_CASES = [(name, hq, hk, d, dt) for name in FAMILIES for (hq, hk) in FAMILY_HEADS for d in DIMS for dt in DTYPES]


@pytest.mark.parametrize("name,hq,hk,d,dtype", FAMILY_CASES, ids=[f"{name}-{hq}x{hk}-d{d}-{tag(dt)}" for name, hq, hk, d, dt in FAMILY_CASES])
def test_value_families(name, hq, hk, d, dtype):
    """peaked, sink, rising, falling and large_v (tests/attn_decode_cases.py; premises in tests/test_attn_decode_inputs_cpu.py) over T + 1
    keys, one key more than a middle split boundary and L_max, in a cache that is NaN behind them, against `bound`; rising and falling
    once more with the last key appended.  `e_kernel <= e_eager` is kept for peaked and large_v only: on sink, rising and falling
    eager's weights round to exactly 1 and 0 in the activation type, its output is then a V row and its error can be exactly 0 -- "no
    worse than eager" is there a criterion that no fp32 kernel can be held to."""
    lmax, geo = geometry(1, hq, hk, d)
    for n in family_lengths(lmax, geo):
        q, k, v, scaling = family_inputs(name, hq, hk, d, dtype, n)
        ref = oracle(q, k, v, n, scaling)
        e32, _ = fp32_error(q, k, v, n, scaling, ref)
        kd = torch.full((1, hk, lmax, d), float("nan"), dtype=dtype, device=DEV)
        vd = kd.clone()
        kd[:, :, :n], vd[:, :, :n] = k.to(DEV), v.to(DEV)
        qd = q[:, :, None].to(DEV)
        got = ops.attn_decode(qd, kd, vd, n, scaling=scaling)
        e_kernel = held(got.cpu(), ref, e32, dtype, f"family {name} {hq}x{hk} d={d} {tag(dtype)} kv_len={n}")
        if name in ("peaked", "large_v"):
            e_eager = (eager(q, k, v, n, scaling).double() - ref).abs().max().item()
            assert e_kernel <= e_eager, (n, e_kernel, e_eager)
        if name in ("rising", "falling"):
            k1, v1 = kd.clone(), vd.clone()
            k1[:, :, n - 1], v1[:, :, n - 1] = float("nan"), float("nan")
            app = ops.attn_decode(qd, k1, v1, dev_len(n - 1), k[:, :, None, n - 1].to(DEV), v[:, :, None, n - 1].to(DEV), scaling=scaling)
            assert same(app, got) and same(k1, kd) and same(v1, vd), n


# ---- 6. memory --------------------------------------------------------------------------------------------------------------------------------
MEMORY_CASES = [(hq, hk, d, b, dt) for (hq, hk) in ((28, 4), (8, 1)) for d in DIMS for b in BATCHES for dt in DTYPES]


def bands_are_nan(buf, view):
    lead = (buf.numel() - view.numel()) // 2
    return bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + view.numel():]).all())


@pytest.mark.parametrize("hq,hk,d,b,dtype", MEMORY_CASES, ids=[f"{hq}x{hk}-d{d}-b{b}-{tag(dt)}" for hq, hk, d, b, dt in MEMORY_CASES])
def test_guard_bands_and_a_dirty_workspace(hq, hk, d, b, dtype):
    """q, k_new, v_new, an additive mask, out and both caches between bands of NaN (gpu_util.guarded), an append at kv_len = 0, behind a
    middle split boundary and into the last position but one: every band stays NaN, every input keeps its bits, the caches change in the
    appended row only, and the output is that of the plain call.  Then everything behind the counter page of the stream's workspace is
    0xFF (fp32 NaN in every partial result of an earlier call): the same bits, twice, and a clean counter page after each call."""
    lmax, geo = geometry(b, hq, hk, d)
    c = normal_inputs(b, hq, hk, d, dtype, lmax, 43)
    pos = torch.arange(lmax, dtype=torch.float64)
    mask = torch.stack([(-((pos + i) % 5) / 4).masked_fill((pos + i) % 7 == 3, float("-inf")) for i in range(b)]).to(dtype)[:, None, None, :].to(DEV)
    ws = ops.workspace(torch.device(DEV), 0)
    try:
        for n in (0, mid_split(geo) * geo["chunk"], lmax - 2):
            k0, v0 = c["kd"].clone(), c["vd"].clone()
            want = ops.attn_decode(c["qd"], k0, v0, n, c["knd"], c["vnd"], mask=mask)
            assert counters_clean()
            held_in = {name: guarded(t) for name, t in (("q", c["qd"]), ("kn", c["knd"]), ("vn", c["vnd"]), ("mask", mask), ("k", c["kd"]), ("v", c["vd"]))}
            held_in["out"] = guarded(torch.full((b, hq, d), float("nan"), dtype=dtype, device=DEV))
            g = {name: view for name, (_, view) in held_in.items()}
            got = ops.attn_decode(g["q"], g["k"], g["v"], n, g["kn"], g["vn"], mask=g["mask"], out=g["out"])
            assert same(got, want), n
            for name, (buf, view) in held_in.items():
                assert bands_are_nan(buf, view), (n, name)
            assert same(g["q"], c["qd"]) and same(g["kn"], c["knd"]) and same(g["vn"], c["vnd"]) and same(g["mask"], mask), n
            assert same(g["k"], k0) and same(g["v"], v0), n
            k0[:, :, n], v0[:, :, n] = c["kd"][:, :, n], c["vd"][:, :, n]
            assert same(k0, c["kd"]) and same(v0, c["vd"]) and not same(g["k"], c["kd"]), n
            ws[COUNTERS:].fill_(0xFF)
            for call in (1, 2):
                k1, v1 = c["kd"].clone(), c["vd"].clone()
                assert same(ops.attn_decode(c["qd"], k1, v1, n, c["knd"], c["vnd"], mask=mask), want), (n, call)
                assert counters_clean() and same(k1, g["k"]) and same(v1, g["v"]), (n, call)
    finally:
        ws[COUNTERS:].zero_()


# ---- 7. the counter page shared with the split-K linears ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ("attention", "linear"))
def test_attention_and_a_split_k_linear_share_the_counter_page(first):
    """On one stream, four rounds of attn_decode (every split live) and a 4-bit GPTQ linear whose plan is split-K (the skinny-ragged row
    of tests/route_matrix.py), in both orders: every output equals its first, and the counter page is zero after each call."""
    import route_matrix as RM
    from route_calls import _descriptor
    r = next(r for r in RM.ROWS if r.id == "skinny-ragged")
    assert r.kind == "GPTQ" and r.bits == 4 and not r.knobs
    layer = to_layer(synth("GPTQ", r.bits, r.g, r.K, r.N, r.zk, r.act_order, r.bias, seed=5), DEV)
    w, keep = _descriptor(r, layer)
    plan = ops.plan_describe([w], r.M)
    assert plan == r.plan and parse_split_k(plan) > 1, plan
    x = torch.from_numpy(randx(r.M, r.K, seed=6)).to(DEV)
    hq, hk, d, dtype = 28, 4, 128, torch.float16
    lmax, geo = geometry(1, hq, hk, d)
    c = normal_inputs(1, hq, hk, d, dtype, lmax, 47)
    assert geo["splits"] > 8 and ops.workspace(torch.device(DEV), 0).data_ptr() == ops.workspace(torch.device(DEV), 1 << 20).data_ptr()
    calls = {"attention": lambda: ops.attn_decode(c["qd"], c["kd"], c["vd"], lmax), "linear": lambda: ops.linear_forward(w, x)}
    order = (first, "linear" if first == "attention" else "attention")
    firsts = {}
    for rnd in range(4):
        for name in order:
            y = calls[name]()
            assert counters_clean(), (rnd, name)
            assert same(y, firsts.setdefault(name, y)), (rnd, name)
    assert bool(torch.isfinite(firsts["attention"]).all()) and bool(torch.isfinite(firsts["linear"]).all())


def parse_split_k(plan):
    import re
    m = re.search(r"split_k=(\d+)", plan)
    return int(m.group(1)) if m else 0
