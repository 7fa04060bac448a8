"""No GPU: the premises of tests/test_attn_prefill_gpu.py, proved on the inputs themselves at every shape, type and offset the GPU file runs
them at (tests/attn_prefill_cases.py).

Selection: pi is visible under causality and not monotone; V's rows differ from each other; the winner leads every other key by more than
40 in the log2 domain; the float64 oracle AND the fp32 restatement of the kernel's arithmetic (`kernel32`: fp32 scores, P rounded to the
type, fp32 sums) round to V[pi(i)] exactly.  Uniform: the oracle IS the mean over the visible keys and `kernel32` rounds to within 1 ulp of it, and every case the GPU
file names (dead rows, a wholly hidden key tile) is really there.  Random values: finite inputs, and `kernel32` rounded to the type sits
inside `bound` -- the tolerance is wide enough for the arithmetic it describes, with the hardware's share (factor 8) to spare."""
import pytest
import torch

from attn_prefill_cases import (DIMS, DTYPES, GROUPS, SEL_GAP_LOG2, SEL_SCALING, U, as_mask, bound, kernel32, oracle, selection,
                                selection_expected, selection_pi, tiles, ulp, uniform, uniform_expected, value_rows, visibility)

from qllm_amd import _lib

pytestmark = pytest.mark.skipif(not _lib.is_built(), reason="library not built")   # the tile sizes come from qllm_attn_prefill_describe


def tag(dtype):
    return str(dtype)[6:]


types = pytest.mark.parametrize("dtype", DTYPES, ids=tag)
dims = pytest.mark.parametrize("d", DIMS)


def selection_shapes(d):
    qt, kt = tiles(d=d)
    return [(s, q_start) for s in (2, 3, qt - 1, qt, qt + 1, 2 * qt + 1) for q_start in (0, 1, kt - 1, kt, kt + 3)]


def test_the_selection_map_is_visible_and_not_monotone():
    for d in DIMS:
        for s, q_start in selection_shapes(d):
            pi = selection_pi(3, 8, s, q_start)
            assert pi.shape == (3, 8, s) and int(pi.min()) >= 0 and bool((pi <= q_start + torch.arange(s)).all())
            if s >= 8:
                assert bool(((pi[..., 1:] < pi[..., :-1]).sum(-1) >= s // 4).all())            # it falls at a quarter of its steps at least
                assert len({tuple(pi[0, h].tolist()) for h in range(8)}) == 8                   # and differs from head to head


@types
def test_value_rows_are_exact_and_tell_every_key_apart(dtype):
    v = value_rows(3, 2, 400, 64, dtype)
    assert torch.equal(v.double(), v.double().round()) and float(v.abs().max()) <= 256              # integers, exact in both types
    rows = v[0, 0].double()
    assert all(len(set(rows[:, c].tolist())) == 400 for c in range(64))                             # distinct in j at every column
    assert all(len(set(r.tolist())) == 64 for r in rows)                                            # distinct in d within every row
    assert not torch.equal(v[0, 0], v[0, 1]) and not torch.equal(v[0, 0], v[1, 0])
    assert float(rows.mean().abs()) > 1                                                             # asymmetric


@pytest.mark.parametrize("hq,hk", GROUPS)
@dims
@types
def test_selection_inputs_select_exactly_in_float64_and_in_the_kernels_arithmetic(dtype, d, hq, hk):
    assert SEL_GAP_LOG2 >= 40
    for b in (1, 3):
        for s, q_start in selection_shapes(d):
            if b == 3 and s > 3 and q_start not in (1, tiles(d=d)[1]):
                continue                                                                            # (the batch changes pi and V by an offset only)
            n = q_start + s
            q, k, v, pi, scaling = selection(b, hq, hk, d, s, q_start, dtype)
            assert scaling == SEL_SCALING and all(torch.equal(t.double().to(dtype), t) for t in (q, k, v))
            sc = torch.einsum("bhsd,bhnd->bhsn", q.double(), k.double().repeat_interleave(hq // hk, dim=1)) * scaling * 1.4426950408889634
            win = torch.gather(sc, 3, pi[..., None])
            rest = sc.scatter(3, pi[..., None], float("-inf")).amax(dim=-1, keepdim=True)
            assert bool((win - rest >= 40).all())
            want = selection_expected(v, pi, hk)
            assert torch.equal(oracle(q, k, v, n, scaling).to(dtype), want)
            assert torch.equal(kernel32(q, k, v, n, scaling).to(dtype), want)


@pytest.mark.parametrize("hq,hk", ((8, 2), (7, 1)))
@dims
@types
def test_uniform_inputs_give_the_mean_of_the_visible_keys(dtype, d, hq, hk):
    from test_attn_prefill_gpu import uniform_masks
    b = 2
    qt, kt = tiles(b, hq, hk, d)
    seen = set()
    for s, q_start in ((qt + 1, 2 * kt + 3), (3, kt), (2 * qt + 1, 0), (qt - 1, kt - 1)):
        n = q_start + s
        q, k, v = uniform(b, hq, hk, d, s, n, dtype, lmax=n + 6)
        assert not bool(q.any()) and bool(torch.isfinite(k).all())
        for name, (vis_mask, causal) in uniform_masks(b, s, n, n + 6, kt, dtype).items():
            for kind in ("bool", "additive") if vis_mask is not None else (None,):
                mask = None if kind is None else as_mask(vis_mask[:, None], kind, dtype)
                vis, bias = visibility(b, s, n, causal, mask)
                assert not bool(bias.any())
                want, cnt = uniform_expected(v, vis, hq)
                if int((cnt == 0).sum()):
                    seen.add("dead")
                if n > 2 * kt and not bool(vis[:, :, kt:2 * kt].any()):
                    seen.add("hidden tile")
                if not causal and bool(vis[:, 0, n - s + 1:].any()):
                    seen.add("above the diagonal")
                o64 = oracle(q, k, v, n, d ** -0.5, causal, mask)                               # the mean itself, to float64's own rounding
                assert bool(((o64 - want).abs() <= 1e-12 * (1 + want.abs())).all()) and bool((o64[cnt == 0] == 0).all()), (name, kind, s, q_start)
                got = kernel32(q, k, v, n, d ** -0.5, causal, mask).to(dtype)
                assert bool(((got.double() - want).abs() <= ulp(want, dtype)).all()) and bool((got[cnt == 0] == 0).all()), (name, kind, s, q_start)
    assert seen == {"dead", "hidden tile", "above the diagonal"}


@pytest.mark.parametrize("name", ("normal", "peaked", "large_v"))
@types
def test_random_inputs_are_finite_and_the_kernels_arithmetic_is_inside_the_bound(dtype, name):
    from test_attn_prefill_gpu import random_case, random_cases
    for d, hq, hk, s, n, masked in random_cases():
        q, k, v, scaling, mask, ref, pv, e32, e_eager = random_case(name, hq, hk, d, dtype, s, n, masked)
        assert q.shape == (1, hq, s, d) and all(bool(torch.isfinite(t).all()) for t in (q, k, v, ref)) and float(v.abs().max()) < 65504
        assert (mask is not None) == masked and e32 > 0 and e_eager > 0 and bool((pv >= ref.abs() - 1e-9).all())
        got = kernel32(q, k, v, n, scaling, True, mask).to(dtype)
        assert bool(((got.double() - ref).abs() <= bound(ref, pv, e32, dtype, factor=1)).all()), (name, d, hq, hk, s, n)
        assert U[dtype] == torch.finfo(dtype).eps / 2
