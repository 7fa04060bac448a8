"""The construction behind tests/test_exact_routes_gpu.py, checked without a GPU and without the library: for every row of the route
matrix and every extra case, at its own layout, bits, group size, zero kind, K and result type, the oracle's W is s (q - z) and both
passes' float64 expectations are representable (the layers are capped at 128 columns here -- the properties are per element; the GPU
test asserts them again at full width before it launches); pass 1 covers every k once, pass 2 reaches every slice of K; the comparison
reports a flipped low bit, a zero point off by one and two swapped rows; and no case is missing from the GPU file."""
import numpy as np
import pytest
import torch

import exact_inputs as E
import route_matrix as RM
import test_exact_routes_gpu as G

N_CAP = 128
ROW = {r.id: r for r in RM.ROWS}
CASES = list(ROW) + list(G.EXTRA)


def _what(cid):
    """(bits, result type, the row counts the GPU test launches with) -- M only moves the launch boundaries"""
    if cid in ROW:
        r = ROW[cid]
        return r.bits, r.dtype, (r.M,)
    _entry, _name, bits, dtype = G.EXTRA[cid]
    return bits, dtype, G.extra_rows(cid)


@pytest.mark.parametrize("cid", CASES)
def test_preconditions_hold(cid):
    first, second = G.row_members(ROW[cid], N_CAP) if cid in ROW else G.extra_members(cid, N_CAP)   # (asserts W == s (q - z), twice)
    bits, dtype, ms = _what(cid)
    K = first[0][0]["K"]
    for d, w in first:
        assert (d["bias"] is None) or dtype == "f16"
        assert set(np.unique(np.log2(d["scales"].astype(np.float64)))) <= set(range(E.EXPONENTS[0], E.EXPONENTS[1] + 1))
        assert np.array_equal(d["z"], np.round(d["z"])) and d["z"].min() >= 0 and d["z"].max() < 2 ** bits
        hot = E.OneHot(K, ms[0], seed=1)
        E.representable(hot.expected(w, d["bias"], hot.ks(0, hot.launches)), dtype)
    nnz = E.sum_nnz(bits, dtype, K)
    assert (nnz < E.MIN_NNZ) == (cid in G.NO_SUMS)
    if G.runs_sums(cid, bits, dtype, K):
        for d, w in second:
            assert d["bias"] is None and bool((d["scales"] == d["scales"][:1]).all())
            x = E.sum_rows(K, 64, nnz, seed=2)
            y = E.sum_expected(w, x)
            E.representable(y, dtype)
            units = (y / torch.from_numpy(d["scales"][0].astype(np.float64))).abs().max()
            assert float(units) <= 2 ** E.SUM_BITS[dtype]


def test_the_listed_sum_exceptions_exist():
    assert set(G.NO_SUMS) <= set(CASES)


@pytest.mark.parametrize("K,M", sorted({(ROW[c].K if c in ROW else G.extra_spec(c)[3], m) for c in CASES for m in _what(c)[2]}))
def test_pass_1_covers_every_k_once(K, M):
    hot = E.OneHot(K, M, seed=K + M)
    assert hot.launches == -(-K // M)
    seen = np.zeros(K, np.int64)
    for j in range(hot.launches):
        ks = hot.ks(j)
        assert len(ks) == M
        x = hot.x(ks).numpy()
        assert x.shape == (M, K)
        rows, cols = np.nonzero(x)
        live = ks >= 0
        assert np.array_equal(rows, np.flatnonzero(live)) and np.array_equal(cols, ks[live])       # one non-zero per live row, at its k
        assert set(x[rows, cols].tolist()) <= set(E.VALUES)
        assert live.all() or j == hot.launches - 1
        np.add.at(seen, ks[live], 1)
    assert bool((seen == 1).all())
    assert set(hot.val.tolist()) == set(E.VALUES)
    if K >= 1024:
        assert not np.array_equal(hot.perm, np.arange(K))


def _k(cid):
    return ROW[cid].K if cid in ROW else G.extra_spec(cid)[3]


@pytest.mark.parametrize("K,nnz", sorted({(_k(c), E.sum_nnz(*_what(c)[:2], _k(c))) for c in CASES if c not in G.NO_SUMS}))
def test_pass_2_puts_one_nonzero_in_every_slice(K, nnz):
    x = E.sum_rows(K, 16, nnz, seed=K + nnz).numpy()
    edges = E.slice_edges(K, nnz)
    assert edges[0] == 0 and edges[-1] == K and bool((np.diff(edges) >= K // nnz).all())
    for a, b in zip(edges[:-1], edges[1:]):
        assert bool((np.count_nonzero(x[:, a:b], axis=1) == 1).all())
    assert set(np.unique(x).tolist()) == {-1.0, 0.0, 1.0}
    assert len({tuple(np.flatnonzero(row)) for row in x}) == 16        # the rows differ


# ---- the comparison, on a numpy stand-in for y ---------------------------------------------------------------------------------------
K0, N0, G0, M0 = 256, 64, 32, 5


def _layer():
    d = E.synth_exact("GPTQ", 4, G0, K0, N0, "asym", False, True, seed=11)
    return d, E.layer_w64(d)


def _stand_in(d, x):
    """what a kernel holding the (possibly damaged) integers of `d` returns: numpy float64, rounded to fp16"""
    w = (d["q"].astype(np.float64) - d["z"].astype(np.float64)[d["g_idx"]]) * d["scales"].astype(np.float64)[d["g_idx"]]
    return torch.from_numpy((x.numpy().astype(np.float64) @ w + d["bias"].astype(np.float64)).astype(np.float16))


def _pass_1(d, w):
    hot = E.OneHot(K0, M0, seed=3)
    ks = hot.ks(0, hot.launches)
    return ks, hot.x(ks), E.representable(hot.expected(w, d["bias"], ks), "f16")


def test_comparison_passes_the_undamaged_layer_and_ignores_the_sign_of_zero():
    d, w = _layer()
    ks, x, want = _pass_1(d, w)
    got = _stand_in(d, x)
    assert E.mismatches(got, want) == (0, [])
    zero = torch.zeros(2, 3, dtype=torch.float16)
    assert E.mismatches(-zero, zero) == (0, [])
    nan = torch.full((2, 3), float("nan"), dtype=torch.float16)
    assert E.mismatches(nan, nan)[0] == 6                       # an element nobody wrote equals nothing


def test_comparison_reports_one_flipped_low_bit():
    d, w = _layer()
    ks, x, want = _pass_1(d, w)
    k, n = 77, 15
    bad = dict(d, q=d["q"].copy())
    bad["q"][k, n] ^= 1
    count, first = E.mismatches(_stand_in(bad, x), want)
    row = int(np.flatnonzero(ks == k)[0])
    assert count == 1 and first[0][:2] == (row, n)
    text = E.describe(d, ks, count, first)
    grp = k // G0
    assert f"({k}, {n}, " in text and text.endswith(f"{int(d['q'][k, n])}, {float(d['z'][grp, n])}, {float(d['scales'][grp, n])})")


def test_comparison_reports_a_zero_point_off_by_one_in_one_group_of_one_column():
    d, w = _layer()
    ks, x, want = _pass_1(d, w)
    grp, n = 3, 14
    bad = dict(d, z=d["z"].copy())
    bad["z"][grp, n] += 1
    count, first = E.mismatches(_stand_in(bad, x), want, limit=K0)
    assert count == G0                                           # every k of that group, in that column, and nothing else
    assert {(int(ks[i]), c) for i, c, _g, _w in first} == {(k, n) for k in range(grp * G0, (grp + 1) * G0)}
    # pass 2 sees it in every row whose +-1 inside that group do not cancel
    x2 = E.sum_rows(K0, 16, 32, seed=4)
    d2 = E.column_scaled(d, seed=5)
    want2 = E.representable(E.sum_expected(E.layer_w64(d2), x2), "f16")
    bad2 = dict(d2, z=bad["z"], bias=np.zeros(N0, np.float16))
    count2, first2 = E.mismatches(_stand_in(bad2, x2), want2, limit=16)
    hit = np.flatnonzero(x2.numpy()[:, grp * G0:(grp + 1) * G0].sum(axis=1) != 0)
    assert count2 == len(hit) > 0 and [(i, c) for i, c, _g, _w in first2] == [(int(i), n) for i in hit]
    assert "row " in E.describe(d2, None, count2, first2)


def test_comparison_reports_two_swapped_rows():
    d, w = _layer()
    ks, x, want = _pass_1(d, w)
    got = _stand_in(d, x)
    a, b = 16, 21                                                # two rows of one 16-row tile and its neighbour
    got[[a, b]] = got[[b, a]]
    count, first = E.mismatches(got, want, limit=4 * N0)
    assert count > N0 and {i for i, _n, _g, _w in first} == {a, b}


# ---- nothing is left out of the GPU file -----------------------------------------------------------------------------------------------
def _parametrised(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    assert any(m.name == "gpu" for m in fn.pytestmark)
    return list(mark.args[1])


def test_every_row_and_every_extra_case_runs_on_the_gpu():
    assert _parametrised(G.test_route_matrix_row_is_exact) == [r.id for r in RM.ROWS]
    assert _parametrised(G.test_unplanned_entry_is_exact) == list(G.EXTRA)
    entries = {G.EXTRA[c][0]: set() for c in G.EXTRA}
    for c, (entry, _name, bits, _dtype) in G.EXTRA.items():
        entries[entry].add(bits)
    assert entries == {"bitpanel": set(G.ALL_BITS), "bitgemm": set(G.ALL_BITS), "bitgroup": set(G.STREAM_BITS), "permuted": set(G.STREAM_BITS)}
    for c in G.EXTRA:                                            # three members of unequal widths; one K for every case
        if G.EXTRA[c][0] == "bitgroup":
            assert len(set(G.extra_spec(c)[4])) == 3
