"""-m gpu: every kernel route, element for element, on layers and activations that have exactly one correct answer (tests/exact_inputs.py).

Every row of the route matrix (tests/route_matrix.py) runs through the C ABI with the row's own shape, knobs, descriptor kind and call,
after its plan string is asserted; the entries the planner does not print (the mid-batch and prefill bit-stream kernels, the grouped
bit-stream matvec, the act-order matvec) run their own smallest ragged and split cases.  Two passes each: a one-hot read-back of every
k (pass 1) and +-1 sums through every K slice (pass 2, on the column-scaled layer).  Before any launch the expectation is checked on
the CPU to be exactly representable (exact_inputs.layer_w64, representable); the comparison is == over every element of every launch,
on the device.  No tolerance anywhere: on these inputs the unrounded-W contract of the strips and the fp16-W contract of the tile GEMMs
name the same number.  The members of a case (`members`) are built without a GPU: tests/test_exact_routes_cpu.py checks them there."""
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import exact_inputs as E
import route_matrix as RM
from route_calls import DEV, _call, _descriptor, _stated_bytes
from test_bitgemm_gpu import CASES as BITGEMM_CASES
from test_bitgemv_actorder_gpu import SHAPES as PERMUTED_SHAPES
from test_bitgemv_group_gpu import CASES as BITGROUP_CASES
from test_bitpanel_gpu import CASES as BITPANEL_CASES

gpu = pytest.mark.gpu
CHUNK_ROWS = 512            # pass 1 at few rows: this many output rows per comparison
WS_BYTES = 64 << 20
ALL_BITS = (2, 3, 4, 5, 6, 7, 8)
STREAM_BITS = (2, 5, 6, 7, 8)      # the widths the grouped and the act-order matvec serve

# Pass 2 needs at least exact_inputs.MIN_NNZ non-zeros per row; the cases below have fewer (a bf16 result holds sums below 2^8 scale
# units: 2 terms at 7 bits, 1 at 8) and run pass 1 only.  tests/test_exact_routes_cpu.py checks that this list is exactly those cases.
NO_SUMS = ("bitgemm-bf16-g32_bias-7", "bitgemm-bf16-g32_bias-8", "bitgemm-bf16-k1216_split-7", "bitgemm-bf16-k1216_split-8")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 100000


# ---- the layers of a case (no GPU) -----------------------------------------------------------------------------------------------------
def members(tag, layout, bits, g, K, widths, zk, bias, act_order, dtype, n_cap=None):
    """([(layer, W)] of pass 1, [(layer, W)] of pass 2), one pair per width: exact layers with the oracle's W in float64, both checked to
    be s (q - z).  `bias`: the index of the one member with a bias, True: all, None / False: none; a bf16 result takes none.  GPTQ
    widths whose zero points do not pack into whole words (N bits % 32 != 0; symmetric only) are synthesised wider and cut, with NULL
    zero points.  `n_cap` (the CPU test): no more than this many columns."""
    def synth(i):
        n = widths[i] if n_cap is None else min(widths[i], n_cap)
        has_bias = dtype != "bf16" and (bias is True or (bias is not None and bias is not False and bias == i))
        whole = layout != "GPTQ" or (n * bits) % 32 == 0
        assert whole or zk == "sym", (tag, n, bits)
        d = E.synth_exact(layout, bits, g, K, n if whole else -(-n // 32) * 32, zk, act_order, has_bias, seed=_seed(tag, i))
        return n, [d, E.column_scaled(d, seed=_seed(tag, i, "sums"))]

    def checked(job):
        n, layer = job
        w = E.layer_w64(layer)
        if n != layer["N"]:
            layer = dict(layer, N=n, qweight=np.ascontiguousarray(layer["qweight"][:, :n]), qzeros=None,
                         scales=np.ascontiguousarray(layer["scales"][:, :n]), q=layer["q"][:, :n], z=layer["z"][:, :n],
                         bias=None if layer["bias"] is None else layer["bias"][:n].copy())
            w = w[:, :n].contiguous()
        return layer, w

    # (the oracle's fp16 arithmetic in numpy is what a wide case spends its time on: the members and the two passes side by side)
    with ThreadPoolExecutor(max_workers=2 * len(widths)) as pool:
        made = list(pool.map(synth, range(len(widths))))
        pairs = list(pool.map(checked, [(n, layer) for n, both in made for layer in both]))
    return pairs[0::2], pairs[1::2]


def row_members(r, n_cap=None):
    return members(r.id, RM.SOURCE_LAYOUT[r.kind], r.bits, r.g, r.K, RM.widths(r), r.zk, r.bias, r.act_order, r.dtype, n_cap)


# The entries the planner does not print: id -> (entry, name of the case in the entry's own test file, bits, dtype).
EXTRA = {}
for _bits in ALL_BITS:
    for _name in ("hqq_ragged", "k1120_split"):          # N = 1000: no multiple of 16; K = 1120: 35 units, two splits of 18 + 17
        EXTRA[f"bitpanel-{_name}-{_bits}"] = ("bitpanel", _name, _bits, "f16")
    for _name in ("g32_bias", "k1216_split"):            # N = 992: 96 live columns in the last tile, a bias; 19 k-tiles: a split of 9 + 10
        EXTRA[f"bitgemm-{_name}-{_bits}"] = ("bitgemm", _name, _bits, "f16")
        EXTRA[f"bitgemm-bf16-{_name}-{_bits}"] = ("bitgemm", _name, _bits, "bf16")
for _bits in STREAM_BITS:
    for _name in ("A", "B"):                             # three members of unequal widths: ragged column blocks / every member splits
        EXTRA[f"bitgroup-{_name}-{_bits}"] = ("bitgroup", _name, _bits, "f16")
    for _name in ("g128", "ragged", "split"):
        EXTRA[f"permuted-{_name}-{_bits}"] = ("permuted", _name, _bits, "f16")
EXTRA["permuted-hqq-8"] = ("permuted", "hqq", 8, "f16")
PERMUTED = dict({k: ("GPTQ", "asym" if k == "g128" else "sym", g, K, N, k == "g128") for k, (g, K, N) in PERMUTED_SHAPES.items()},
                split=("GPTQ", "asym", 64, 4096, 64, True),        # test_two_chunks_of_staged_activations_and_the_k_split's layer
                hqq=("HQQ", "f16", 64, 1024, 256, False))          # test_hqq_zero_points_with_a_random_permutation's


def extra_spec(cid):
    """(layout, zero kind, group, K, widths, bias) of an extra case, from its entry's own CASES"""
    entry, name, _bits, _dtype = EXTRA[cid]
    if entry in ("bitpanel", "bitgemm"):
        layout, g, K, N, zk, bias = (BITPANEL_CASES if entry == "bitpanel" else BITGEMM_CASES)[name]
        return layout, zk, g, K, (N,), bias
    if entry == "bitgroup":
        layout, zk, g, K, widths, biased = BITGROUP_CASES[name]
        return layout, zk, g, K, widths, biased
    layout, zk, g, K, N, bias = PERMUTED[name]
    return layout, zk, g, K, (N,), bias


def extra_rows(cid):
    """the row counts an extra case launches with: the entry's fewest and, for the mid-batch kernel, the most the modules send it"""
    from qllm_amd import _lib
    entry, name, _bits, _dtype = EXTRA[cid]
    if entry == "permuted":
        return (16,) if name == "split" else (1, 3, 16)
    return {"bitpanel": (17, _lib.BITPANEL_MAX_M_DEFAULT), "bitgemm": (129,), "bitgroup": (1, 3)}[entry]


def extra_members(cid, n_cap=None):
    layout, zk, g, K, widths, bias = extra_spec(cid)
    _entry, _name, bits, dtype = EXTRA[cid]
    return members(cid, layout, bits, g, K, widths, zk, bias, False, dtype, n_cap)


def runs_sums(cid, bits, dtype, K):
    """whether pass 2 runs: enough non-zeros, or the case is one of NO_SUMS"""
    enough = E.sum_nnz(bits, dtype, K) >= E.MIN_NNZ
    assert enough != (cid in NO_SUMS), (cid, E.sum_nnz(bits, dtype, K))
    return enough


# ---- the two passes ------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _compare(tag, what, mems, ys, wants, ks):
    for i, ((d, _w), y, want) in enumerate(zip(mems, ys, wants)):
        count, first = E.mismatches(y, want.to(DEV))
        assert count == 0, f"{tag}: {what}, member {i} of {len(mems)}: " + E.describe(d, ks, count, first)


def run_passes(cid, plan, dtype, M, bits, first, second, launch):
    """Both passes of one case.  `launch(which, x, outs)` runs the route on pass `which`'s descriptors: x [M, K] and one [M, N] output per
    member, views into the chunk buffers.  Every expectation is built and checked on the CPU before the first launch."""
    tag = f"{cid} [{plan}]"
    tdt = E.TORCH_DTYPE[dtype]
    K = first[0][0]["K"]
    t0 = time.perf_counter()
    hot = E.OneHot(K, M, seed=_seed(tag, M, "one-hot"))
    per = max(1, CHUNK_ROWS // M)                                  # launches per chunk
    chunks = []
    for at in range(0, hot.launches, per):
        n = min(per, hot.launches - at)
        ks = hot.ks(at, n)
        chunks.append((at, n, ks, [E.representable(hot.expected(w, d["bias"], ks), dtype) for d, w in first]))
    sums = None
    if runs_sums(cid, bits, dtype, K):
        rows = 16 if M == 1 else M
        x2 = E.sum_rows(K, rows, E.sum_nnz(bits, dtype, K), seed=_seed(tag, M, "sums"))
        sums = (x2, [E.representable(E.sum_expected(w, x2), dtype) for _d, w in second])
    t1 = time.perf_counter()

    xbuf = torch.empty(per * M, K, dtype=tdt, device=DEV)
    ybufs = [torch.empty(per * M, d["N"], dtype=tdt, device=DEV) for d, _w in first]
    for at, n, ks, wants in chunks:
        xbuf[:n * M].copy_(hot.x(ks).to(tdt))
        for y in ybufs:
            y.fill_(float("nan"))
        for j in range(n):
            launch(1, xbuf[j * M:(j + 1) * M], [y[j * M:(j + 1) * M] for y in ybufs])
        _compare(tag, f"pass 1, launches {at}..{at + n - 1} of {M} rows", first, [y[:n * M] for y in ybufs], wants, ks)
    if sums is not None:
        x2, wants = sums
        xs = _dev(x2.numpy(), tdt)
        ys = [torch.full((x2.shape[0], d["N"]), float("nan"), dtype=tdt, device=DEV) for d, _w in second]
        for j in range(0, x2.shape[0], M):
            launch(2, xs[j:j + M], [y[j:j + M] for y in ys])
        _compare(tag, f"pass 2, {x2.shape[0]} rows of {E.sum_nnz(bits, dtype, K)} non-zeros", second, ys, wants, None)
    torch.cuda.synchronize()
    print(f"{tag}: {hot.launches} + {0 if sums is None else -(-sums[0].shape[0] // M)} launches; expectations {t1 - t0:.2f} s, "
          f"GPU passes {time.perf_counter() - t1:.2f} s")


# ---- every row of the route matrix -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rid", [r.id for r in RM.ROWS])
def test_route_matrix_row_is_exact(rid):
    from gpu_util import to_layer
    from qllm_amd import ops
    r = next(r for r in RM.ROWS if r.id == rid)
    first, second = row_members(r)
    layers = [[to_layer(d, DEV) for d, _w in mems] for mems in (first, second)]
    descs = [[_descriptor(r, layer)[0] for layer in ls] for ls in layers]
    try:
        for k, v in r.knobs.items():
            ops.set_knob(k, v)
        for ds in descs:
            assert ops.plan_describe(ds, r.M) == r.plan, r.id
        ws = torch.zeros(max(WS_BYTES, _stated_bytes(r, descs[0])), dtype=torch.uint8, device=DEV)
        run_passes(r.id, r.plan, r.dtype, r.M, r.bits, first, second,
                   lambda which, x, outs: _call(descs[which - 1], x, outs, ws.data_ptr(), ws.numel()))
    finally:
        ops.reset_knobs()


# ---- the entries the planner does not print --------------------------------------------------------------------------------------------
def _weights(mems):
    from qllm_amd import ops
    out = []
    for d, _w in mems:
        qz = None if d["qzeros"] is None or (d["layout"] == "GPTQ" and bool((d["z"] == 2 ** (d["bits"] - 1)).all())) else _dev(d["qzeros"])
        out.append(ops.make_weight(d["layout"], _dev(d["qweight"]), _dev(d["scales"]), qz, None, None if d["bias"] is None else _dev(d["bias"]),
                                   d["K"], d["N"], d["groupsize"], d["bits"], 0))
    return [w for w, _keep in out], [keep for _w, keep in out]


def _split_of(text):
    return [int(v) for v in text.rsplit("split_k=", 1)[1].split(",")]


@gpu
@pytest.mark.parametrize("cid", list(EXTRA))
def test_unplanned_entry_is_exact(cid):
    from qllm_amd import ops
    entry, name, bits, dtype = EXTRA[cid]
    first, second = extra_members(cid)
    descs, _keep = zip(*(_weights(mems) for mems in (first, second)))
    K = first[0][0]["K"]
    wide = torch.cuda.get_device_properties(0).multi_processor_count >= 128     # (the split rules count the device's CUs)
    if entry == "bitpanel":
        assert extra_rows(cid)[1] == ops.bitpanel_max_m()
        for m in extra_rows(cid):
            text = ops.bitpanel_describe(descs[0][0], m)
            assert text.startswith(f"bitpanel bits={bits} ") and 17 <= m <= 512, text
            assert _split_of(text)[0] > 1 or not name.endswith("_split"), text
            run_passes(cid, text, dtype, m, bits, first, second,
                       lambda which, x, outs: ops.linear_forward_bitpanel(descs[which - 1][0], x, out=outs[0]))
    elif entry == "bitgemm":
        (m,) = extra_rows(cid)
        text = ops.bitgemm_describe(descs[0][0], m)
        assert text.startswith(f"bitgemm bits={bits} "), text
        if wide:
            assert _split_of(text)[0] > 1 or not name.endswith("_split"), text
        run_passes(cid, text, dtype, m, bits, first, second,
                   lambda which, x, outs: ops.linear_forward_bitgemm(descs[which - 1][0], x, out=outs[0]))
    elif entry == "bitgroup":
        assert len(descs[0]) == 3 and len({w.N for w in descs[0]}) == 3
        for m in extra_rows(cid):
            text = ops.bitgroup_describe(list(descs[0]), m)
            assert text.startswith(f"bitgroup bits={bits} "), text
            assert all((s > 1) == (name == "B") for s in _split_of(text)), text
            run_passes(cid, text, dtype, m, bits, first, second,
                       lambda which, x, outs: ops.linear_forward_bitgroup(list(descs[which - 1]), x, outs))
    else:
        # y = x[:, perm] . W: the activations of the plain layer, scattered to where the permutation fetches them from
        perm = np.random.default_rng(_seed(cid, "perm")).permutation(K).astype(np.int32)
        pt = _dev(perm)
        inverse = _dev(np.argsort(perm))
        for m in extra_rows(cid):
            text = ops.plan_describe([descs[0][0]], m)
            assert text.startswith(f"bitgemv bits={bits} "), text
            assert (_split_of(text)[0] > 1) or name != "split", text
            run_passes(cid, "permuted " + text, dtype, m, bits, first, second,
                       lambda which, x, outs: ops.linear_forward_permuted(descs[which - 1][0], pt, x.index_select(1, inverse), out=outs[0]))
