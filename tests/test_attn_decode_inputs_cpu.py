"""No GPU: the premises of tests/test_attn_decode_edges_gpu.py, proved on the inputs themselves -- the tolerance `bound`, the value families
(tests/attn_decode_cases.py) at every shape, type and length the GPU file runs them at, and the masks' arithmetic in the oracle.

Per family, type, shape and length: the float64 oracle is finite and fits the type; in at least half of the (batch, head) rows at least two
keys carry a weight above 2^-24 (no one-key-wins case in disguise); `rising` / `falling`: the per-tile maximum of the float64 scores
strictly increases / decreases over at least 3/4 of the tile boundaries of every row; `sink`: the five pulled positions score 20 to 40
above the bulk's largest; and the fp32 restatement of the op, rounded once, stays within `bound` with factor 1 -- the reference has room
under the factor 8 the kernel is held to.  The lengths follow the launch geometry (qllm_attn_decode_describe), which is pure host code."""
import pytest
import torch

from attn_decode_cases import (DIMS, DTYPES, FAMILIES, FAMILY_HEADS, SINK_SCORES, bound, family_inputs, family_lengths, fp32_error, geometry, halfulp,
                               oracle, restated, restated32, scores64)

from qllm_amd import _lib

CASES = [(name, hq, hk, d, dt) for name in FAMILIES for (hq, hk) in FAMILY_HEADS for d in DIMS for dt in DTYPES]
IDS = [f"{name}-{hq}x{hk}-d{d}-{str(dt)[6:]}" for name, hq, hk, d, dt in CASES]


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("library not built")
    return _lib.load()


def test_halfulp_is_half_the_spacing_of_the_type():
    for dtype, mant, emin in ((torch.float16, 10, -14), (torch.bfloat16, 7, -126)):
        x = torch.tensor([1.0, 1.5, -1.999, 2.0, 1000.0, 0.3, 2.0 ** emin, 2.0 ** (emin - 3), 0.0], dtype=torch.float64)
        want = [2.0 ** (-mant - 1)] * 3 + [2.0 ** (-mant), 2.0 ** (9 - mant - 1), 2.0 ** (-2 - mant - 1)] + [2.0 ** (emin - mant - 1)] * 3
        assert halfulp(x, dtype).tolist() == want, dtype
        # one rounding of any fp32 value of the type's range costs at most halfulp of that value
        gen = torch.Generator().manual_seed(1)
        v = torch.randn(20000, generator=gen, dtype=torch.float64) * torch.tensor(2.0, dtype=torch.float64) ** torch.randint(-16, 14, (20000,), generator=gen)
        v = v.float().double()
        assert bool(((v.to(dtype).double() - v).abs() <= halfulp(v, dtype)).all()), dtype
    assert halfulp(torch.zeros(1, dtype=torch.float64), torch.float16).item() == 2.0 ** -25
    assert halfulp(torch.zeros(1, dtype=torch.float64), torch.bfloat16).item() == 2.0 ** -134
    ref = torch.tensor([0.75], dtype=torch.float64)
    assert bound(ref, 1e-6, torch.float16).item() == 2.0 ** -12 + 8e-6 and bound(ref, 1e-6, torch.float16, factor=1).item() == 2.0 ** -12 + 1e-6


def test_restated_is_restated32_rounded_once():
    gen = torch.Generator().manual_seed(2)
    q, k, v = torch.randn(2, 6, 1, 64, generator=gen).half(), torch.randn(2, 2, 40, 64, generator=gen).half(), torch.randn(2, 2, 40, 64, generator=gen).half()
    kn, vn = torch.randn(2, 2, 1, 64, generator=gen).half(), torch.randn(2, 2, 1, 64, generator=gen).half()
    mask = torch.rand(2, 1, 1, 40, generator=gen) > 0.3
    k1, v1, k2, v2 = k.clone(), v.clone(), k.clone(), v.clone()
    a32 = restated32(q, k1, v1, 17, kn, vn, mask, 0.2)
    a = restated(q, k2, v2, 17, kn, vn, mask, 0.2)
    assert a32.dtype == torch.float32 and a.dtype == torch.float16 and torch.equal(a32.half(), a)
    assert torch.equal(k1, k2) and torch.equal(k1[:, :, 17], kn[:, :, 0]) and torch.equal(v1[:, :, 17], vn[:, :, 0])


def test_the_oracle_adds_a_bias_and_hides_what_is_not_visible():
    gen = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(2, 4, 64, generator=gen), torch.randn(2, 2, 30, 64, generator=gen), torch.randn(2, 2, 30, 64, generator=gen)
    visible = torch.rand(2, 30, generator=gen) > 0.4
    bias = torch.randn(2, 30, generator=gen)
    by_hand = torch.stack([torch.stack([torch.softmax((k[b, h // 2, :25].double() @ q[b, h].double()) * 0.3 + bias[b, :25].double()
                                                      + torch.where(visible[b, :25], 0.0, float("-inf")).double(), 0) @ v[b, h // 2, :25].double()
                                        for h in range(4)]) for b in range(2)])
    assert torch.allclose(oracle(q, k, v, 25, 0.3, visible, bias), by_hand, rtol=0, atol=1e-13)
    minus_inf = bias.masked_fill(~visible, float("-inf"))
    assert torch.equal(oracle(q, k, v, 25, 0.3, None, minus_inf), oracle(q, k, v, 25, 0.3, visible, bias))
    assert torch.equal(oracle(q, k, v, 25, 0.3, visible[:1], bias[:1]), oracle(q, k, v, 25, 0.3, visible[:1].expand(2, 30), bias[:1].expand(2, 30)))


@pytest.mark.parametrize("name,hq,hk,d,dtype", CASES, ids=IDS)
def test_family_premises(lib, name, hq, hk, d, dtype):
    lmax, geo = geometry(1, hq, hk, d)
    tile = geo["tile"]
    for n in family_lengths(lmax, geo):
        q, k, v, scaling = family_inputs(name, hq, hk, d, dtype, n)
        assert q.dtype == k.dtype == v.dtype == dtype and q.shape == (1, hq, d) and k.shape == v.shape == (1, hk, n, d)
        ref = oracle(q, k, v, n, scaling)
        assert bool(torch.isfinite(ref).all()) and ref.abs().max().item() <= torch.finfo(dtype).max, (n, "the oracle must fit the type")
        s = scores64(q, k, n, scaling).reshape(hq, n)
        w = torch.softmax(s, dim=-1)
        rows = (w > 2.0 ** -24).sum(dim=-1) >= 2
        assert 2 * int(rows.sum()) >= hq, (n, "one key wins in more than half of the rows", rows.tolist())
        if name in ("rising", "falling"):
            tiles = torch.stack([s[:, a:a + tile].max(dim=-1).values for a in range(0, n, tile)], dim=-1)      # [Hq, tiles]
            step = tiles[:, 1:] - tiles[:, :-1]
            good = (step > 0 if name == "rising" else step < 0).sum(dim=-1)
            assert tiles.shape[1] >= 2 and bool((4 * good >= 3 * step.shape[1]).all()), (n, good.tolist(), step.shape[1])
            assert 0.9 * 30 * (n - 1) / n <= (s.max(dim=-1).values - s.min(dim=-1).values).min().item() and (s.max() - s.min()).item() <= 31
        if name == "sink":
            pulled = sorted({0} | set(range(max(0, n - 4), n)))
            bulk = s[:, [p for p in range(n) if p not in pulled]].max(dim=-1, keepdim=True).values
            above = s[:, pulled] - bulk
            assert len(pulled) == len(SINK_SCORES) and 20 <= above.min().item() and above.max().item() <= 40, (n, above.min().item(), above.max().item())
        if name == "peaked":
            assert 6 <= s.std().item() <= 10, (n, s.std().item())
        if name == "large_v":
            assert 900 <= v.abs().max().item() <= 1024 and 0.7 <= s.std().item() <= 1.4
        e32, r32 = fp32_error(q, k, v, n, scaling, ref)
        worst = ((r32.to(dtype).double() - ref).abs() / bound(ref, e32, dtype, factor=1)).max().item()
        assert worst <= 1.0, (n, worst, e32)
        # the fp32 term of the bound the kernel is held to is at most a quarter of the rounding term at the largest output
        assert 8 * e32 <= halfulp(ref.abs().max().reshape(1), dtype).item() / 4, (n, e32)
