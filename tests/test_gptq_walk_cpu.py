"""The float32 walk of tests/gptq_walk_cases.py, the oracle of tests/test_gptq_walk_gpu.py, checked without a GPU and without the library:
against the fixtures minted from the reference (tests/golden/gptq_quant, tests/golden/gptq_static), against eight deliberate mistakes
(each must change something that the GPU tests compare, on a case of the matrix), and for the premises of every case.

Measured figures: profiles/gptq_quantize.md."""
import glob
import os

import numpy as np
import pytest
import torch

import gptq_walk_cases as C
from gptq_walk_cases import F, BLK, find_params, group_table, lane_of

HERE = os.path.dirname(os.path.abspath(__file__))
DYN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "gptq_quant", "gptqq_*.npz")))
STA = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "gptq_static", "gptqs_*.npz")))
IDS = [c["id"] for c in C.CASES]


# ---- the oracle against the reference's fixtures ------------------------------------------------------------------------------------------
def fixture(sub, name):
    d = dict(np.load(os.path.join(HERE, "golden", sub, name + ".npz"), allow_pickle=False))
    for k in ("bits", "groupsize", "N", "K", "sym", "act_order"):
        d[k] = int(d[k])
    X = d["X"].reshape(-1, d["K"]).astype(np.float64)
    d["H64"] = 2.0 / d["X"].shape[0] * (X.T @ X)
    Wz = d["W"].astype(np.float64).copy()
    Wz[:, np.diag(d["H64"]) == 0] = 0                # dead columns: the reference zeroes them before anything else
    d["Wz"] = Wz
    return d


def check_quality(d, name, codes_nk, loss, wq, first):
    """The kernel tier's bounds of test_gptq_quantize_gpu.py / test_gptq_static_gpu.py; codes_nk / wq in the original column order, `first`
    the original columns of the first 128 processed."""
    diff = codes_nk != d["codes"]
    D = d["Wz"] - wq.astype(np.float64)
    e = float(np.einsum("nk,kj,nj->", D, d["H64"], D))
    print(f"oracle {name}: codes differ {int(diff.sum())} of {diff.size} (first 128 columns {int(diff[:, first].sum())}); loss {loss:.6e} vs "
          f"{d['error']:.6e} (x{loss / d['error']:.5f}); out err {e:.6e} vs gptq {d['gptq_out_err']:.6e} (x{e / d['gptq_out_err']:.5f}) "
          f"rtn {d['rtn_out_err']:.6e}")
    assert diff.mean() <= 0.01
    assert not diff[:, first].any()
    assert loss <= 1.01 * d["error"]
    assert e <= 1.01 * d["gptq_out_err"]
    assert e < 0.5 * (d["gptq_out_err"] + d["rtn_out_err"])


def test_all_sixteen_fixtures_are_present():
    assert len(DYN) == 10 and len(STA) == 6


@pytest.mark.parametrize("name", DYN)
def test_oracle_matches_the_reference_dynamic_groups(name):
    d = fixture("gptq_quant", name)
    perm, dt = d["perm"], C.DTYPES[str(d["w_dtype"])]
    W = d["Wz"][:, perm].astype(F)
    assert np.array_equal(torch.from_numpy(W).to(dt).float().numpy(), W)
    codes, scale, zero, dq, _, loss = C.walk(W, d["U"], None, d["bits"], d["groupsize"], bool(d["sym"]), False)
    assert np.array_equal(scale[:, 0], d["scale"][:, 0]) and np.array_equal(zero[:, 0], d["zero"][:, 0])      # group 0: from W alone
    inv = np.argsort(perm)
    wq = torch.from_numpy(dq).to(dt).float().numpy()                                                           # as the kernel stores it
    check_quality(d, name, codes[:, inv], float(loss.astype(np.float64).sum()), wq[:, inv], perm[:128])


@pytest.mark.parametrize("name", STA)
def test_oracle_matches_the_reference_static_groups(name):
    d = fixture("gptq_static", name)
    dt = C.DTYPES[str(d["w_dtype"])]
    W = d["Wz"].astype(F)
    assert np.array_equal(torch.from_numpy(W).to(dt).float().numpy(), W)
    perm = d["perm"] if d["act_order"] else None
    codes, scale, zero, dq, _, loss = C.walk(W, d["U"], perm, d["bits"], d["groupsize"], bool(d["sym"]), True)
    assert np.array_equal(scale, d["scale"]) and np.array_equal(zero, d["zero"])                               # every group: from W alone
    wq = torch.from_numpy(dq).to(dt).float().numpy()
    check_quality(d, name, codes, float(loss.astype(np.float64).sum()), wq, d["perm"][:128])


# ---- teeth: the oracle with one mistake -----------------------------------------------------------------------------------------------------
def fms(c, a, b):
    """c - a * b with the product kept exact (float64 holds it) and one rounding of the difference to float64, then float32: a contracted
    multiply-subtract, near enough."""
    return (c.astype(np.float64) - a.astype(np.float64) * b.astype(np.float64)).astype(F)


MISTAKES = ("fused in-block update", "fused trailing update", "earlier blocks in reverse", "times the reciprocal", "floor(x + 0.5)",
            "parameters column by column", "static table from the updated state", "perm applied to U")


def mistaken(W, U, perm, bits, g, sym, static, mistake=None):
    """A copy of gptq_walk_cases.walk that makes `mistake` (None: none)."""
    assert mistake is None or mistake in MISTAKES
    W = np.ascontiguousarray(W)
    N, K = W.shape
    G, maxq = K // g, F(2 ** bits - 1)
    if U is None:
        perm = None
    col_of = np.arange(K) if perm is None else np.asarray(perm, dtype=np.int64)
    if mistake == "perm applied to U" and U is not None:
        U = np.ascontiguousarray(U[col_of][:, col_of])
    shift = 31 if g == K else g.bit_length() - 1
    Wp = W[:, col_of]
    if static or g == K:
        scale, zero = group_table(W, g, maxq, sym)
    else:
        scale, zero = np.zeros((N, G), F), np.zeros((N, G), F)
    current = W.copy()                                          # ("static table from the updated state": what W has become)
    codes, dq, err = np.zeros((N, K), np.int32), np.zeros((N, K), F), np.zeros((N, K), F)
    lanes = np.zeros((N, 16), F)
    round_ = (lambda v: np.floor(v + F(0.5))) if mistake == "floor(x + 0.5)" else np.rint

    for i1 in range(0, K, BLK):
        cnt = min(BLK, K - i1)
        w = Wp[:, i1:i1 + cnt].copy()
        if U is not None:
            earlier = list(range(0, i1, BLK))
            for p1 in earlier[::-1] if mistake == "earlier blocks in reverse" else earlier:
                acc = np.zeros((N, cnt), F)
                for k in range(p1, p1 + BLK):
                    if mistake == "fused trailing update":
                        acc = fms(acc, -err[:, k, None], U[None, k, i1:i1 + cnt])
                    else:
                        acc = acc + err[:, k, None] * U[None, k, i1:i1 + cnt]
                w = w - acc
        if not static and g != K:
            s, z = group_table(w, g, maxq, sym)
            scale[:, i1 // g:i1 // g + cnt // g], zero[:, i1 // g:i1 // g + cnt // g] = s, z
        if static and mistake == "static table from the updated state":
            current[:, col_of[i1:i1 + cnt]] = w
            scale, zero = group_table(current, g, maxq, sym)
        grp = (col_of[i1:i1 + cnt] >> shift) if static else (np.arange(i1, i1 + cnt) >> shift)
        for i in range(cnt):
            if mistake == "parameters column by column" and not static and g != K and i % g == 0:
                v = w[:, i:i + g]
                scale[:, grp[i]], zero[:, grp[i]] = find_params(np.minimum(v.min(1), F(0)), np.maximum(v.max(1), F(0)), maxq, sym)
            s, z = scale[:, grp[i]], zero[:, grp[i]]
            x = w[:, i]
            q = np.minimum(np.maximum(round_(x / s) + z, F(0)), maxq)
            y = s * (q - z)
            diff = x - y
            if U is None:
                ev, term = np.zeros(N, F), diff * diff
            else:
                d = U[i1 + i, i1 + i]
                ev = diff * (F(1) / d) if mistake == "times the reciprocal" else diff / d
                term = (diff * diff) / (d * d)
                if mistake == "fused in-block update":
                    w[:, i + 1:] = fms(w[:, i + 1:], ev[:, None], U[None, i1 + i, i1 + i + 1:i1 + cnt])
                else:
                    w[:, i + 1:] = w[:, i + 1:] - ev[:, None] * U[None, i1 + i, i1 + i + 1:i1 + cnt]
            lanes[:, lane_of(i)] = lanes[:, lane_of(i)] + term
            codes[:, col_of[i1 + i]], dq[:, col_of[i1 + i]], err[:, i1 + i] = q.astype(np.int32), y, ev
    for m in (1, 2, 4, 8):
        lanes = lanes + lanes[:, np.arange(16) ^ m]
    return codes, scale, zero, dq, err, lanes[:, 0] * F(0.5)


NAMES = ("codes", "scale", "zero", "dq", "err", "loss")
# where each mistake is looked for: the cases of the matrix that reach the code it is made in
TEETH = {
    "fused in-block update": ["dyn-N40-K1024-g32-w4a-float16-randn-dense", "dyn-N17-K384-g64-w5a-float32-randn-dense"],
    "fused trailing update": ["dyn-N40-K1024-g32-w4a-float16-randn-dense", "dyn-N40-K416-g32-w4a-float16-randn-dense"],
    "earlier blocks in reverse": ["dyn-N40-K1024-g32-w4a-float16-randn-dense", "dyn-N17-K384-g64-w7a-float32-randn-dense"],
    "times the reciprocal": ["dyn-N40-K1024-g32-w4a-float16-randn-dense", "dyn-N17-K320-g64-w4a-float16-randn-diag"],
    "floor(x + 0.5)": ["dyn-N17-K320-g64-w4a-float16-ties-none", "static-N17-K320-g32-w3a-float16-ties-none"],
    "parameters column by column": ["dyn-N40-K320-g32-w4a-float16-randn-dense", "dyn-N40-K320-g64-w4a-float16-randn-dense"],
    "static table from the updated state": ["static-N17-K256-g32-w4a-float16-randn-dense-random", "static-N17-K320-g64-w4a-float16-dead-dense-diag"],
    "perm applied to U": ["static-N17-K256-g32-w4a-float16-randn-dense-random", "static-N17-K320-g64-w4a-float16-dead-dense-diag"],
}


def differing(a, b):
    """{name: number of elements whose bits differ} over the six outputs."""
    return {n: int((x.view(np.int32) != y.view(np.int32)).sum()) for n, x, y in zip(NAMES, a, b)}


@pytest.mark.parametrize("cid", sorted({i for ids in TEETH.values() for i in ids}))
def test_the_copy_without_a_mistake_is_the_oracle(cid):
    c = C.BY_ID[cid]
    W, U, perm = C.inputs(c)
    got = mistaken(W, U, perm, c["bits"], c["g"], bool(c["sym"]), c["kernel"] == "static")
    assert not any(differing(C.run(c), got).values())


@pytest.mark.parametrize("mistake", MISTAKES)
def test_every_mistake_changes_a_compared_quantity(mistake):
    assert set(TEETH) == set(MISTAKES)
    for cid in TEETH[mistake]:
        c = C.BY_ID[cid]
        W, U, perm = C.inputs(c)
        got = mistaken(W, U, perm, c["bits"], c["g"], bool(c["sym"]), c["kernel"] == "static", mistake)
        n = differing(C.run(c), got)
        print(f"{mistake} | {cid}: differing bits in {n}")
        assert any(n.values()), cid


# ---- premises of the matrix -----------------------------------------------------------------------------------------------------------------
def test_the_matrix_reaches_every_branch():
    dyn, sta = C.DYNAMIC, C.STATIC
    assert len(dyn) == 61 and len(sta) == 43
    assert {(c["bits"], c["sym"]) for c in dyn if c["g"] == 64 and c["K"] == 384} == {(b, s) for b in range(2, 9) for s in (0, 1)}
    assert {(c["K"], c["g"]) for c in dyn} >= {(K, g) for K in (128, 160, 192, 320, 416, 1024) for g in (32, 64, 128, K)
                                               if K % g == 0 and K % 4 == 0}
    assert {c["K"] for c in dyn if c["g"] == c["K"]} >= {4, 100, 252, 640}
    assert {c["N"] for c in dyn if c["K"] == 320 and c["g"] == 64} >= {1, 15, 16, 17, 40}
    assert {(c["dtype"], c["g"] == c["K"], c["sym"]) for c in dyn} >= {(d, r, s) for d in C.DTYPES for r in (False, True) for s in (0, 1)}
    for group in (dyn, sta):
        assert {c["w"] for c in group} == {"randn", "signed", "flat", "outlier", "dead", "ties"}
        assert {c["u"] for c in group} == {"none", "identity", "diag", "dense"}
    assert {c["perm"] for c in sta} == {"none", "reversed", "random", "diag"} and {c["perm"] for c in dyn} == {"none"}
    assert 0.4 * len(dyn) <= len(sta) <= 0.75 * len(dyn)
    assert all(c["K"] % c["g"] == 0 and c["K"] % 4 == 0 and c["g"] in (32, 64, 128, c["K"]) for c in C.CASES)     # what the entries accept


@pytest.mark.parametrize("cid", IDS)
def test_premises_of_the_case(cid):
    c = C.BY_ID[cid]
    W, U, perm = C.inputs(c)
    dt = C.DTYPES[c["dtype"]]
    assert np.array_equal(torch.from_numpy(W).to(dt).float().numpy(), W)                 # exact in the storage type
    stats = {}
    out = C.run(c, stats)
    assert all(np.isfinite(a).all() for a in out[1:])
    assert stats.get("tiny", 1.0) >= C.TINY, stats
    assert stats.get("product", 1.0) >= 2.0 ** -126, stats                                # no product is subnormal either
    codes, scale, zero = out[:3]
    maxq = 2 ** c["bits"] - 1
    assert codes.min() >= 0 and codes.max() <= maxq
    if c["u"] == "dense":
        rtn = C.walk(W, None, None, c["bits"], c["g"], bool(c["sym"]), c["kernel"] == "static")
        assert (rtn[0] != codes).any()
    if c["w"] == "signed":
        assert (zero == 0).any() and (zero == maxq).any() and set(np.unique(zero[:, 0])) == {0.0, float(maxq)}
    if c["w"] == "flat":
        assert (scale == F(2) / F(maxq)).any() and (out[3][0] == 0).all() and (out[5][0] == 0)
    if c["w"] == "outlier":
        assert (np.abs(W).max(1) == 1).all()
    if c["w"] == "ties":
        assert (scale == 1).all() and (zero == 0).all()
        floor = mistaken(W, U, perm, c["bits"], c["g"], bool(c["sym"]), c["kernel"] == "static", "floor(x + 0.5)")
        assert (floor[0] != codes).any()
    if c["w"] == "dead" and U is not None:
        at = C.DEAD(c["K"]) if perm is None else [int(np.nonzero(perm == k)[0][0]) for k in C.DEAD(c["K"])]
        off = U[at].copy()
        off[np.arange(len(at)), at] = 0
        assert (W[:, C.DEAD(c["K"])] == 0).all() and (off == 0).all() and (out[3][:, C.DEAD(c["K"])] == 0).all()


def test_a_lane_meets_eight_different_groups():
    """g = 32 with a random perm over K >= 256: the eight columns of one lane in one block fall into eight different groups."""
    hit = 0
    for c in C.STATIC:
        if c["g"] == 32 and c["perm"] == "random" and c["K"] >= 256 and c["u"] == "dense":
            perm = C.inputs(c)[2]
            for i1 in range(0, c["K"] - BLK + 1, BLK):
                for l in range(16):
                    cols = [i1 + 64 * h + 4 * l + r for h in (0, 1) for r in range(4)]
                    hit += len({int(perm[j]) >> 5 for j in cols}) == 8
    assert hit > 0
