"""-m gpu: RMSNorm standalone (qllm_rmsnorm, csrc/rmsnorm.hip) and fused into the grouped launch of the layers it feeds
(qllm_linear_forward_rmsnorm, csrc/strip1_norm.hip: the NORM forms of the batch-1 kernel), through the C ABI and the modules.

The arithmetic contract of the fused entry is bit identity with the plain grouped launch on xn = w_norm * (x.float() * rstd).to(dtype),
rstd being the value the launch reports; rstd itself is held to float64 within (K/2 + 8) 2^-24 relative: an fp32 sum of K exact
non-negative terms in any order is within (K - 1) 2^-24, divide / add / rsqrt add a few roundings, and rsqrt halves the relative error of
its argument.  Against the eager transformers expression the outputs are held to the project's tolerances (tests/test_strip1_gpu.py) and
the share of outputs whose bits differ from the eager path is printed, not asserted.

Shapes: the smallest at which each mechanism can go wrong -- K = 256 (4 waves x 8, not exact: three waves own nothing and all windows
overlap, the double-count case), 1024 (exact), 3584 (seven waves), 11008 (15 x 24, shifted last window, weight chunks parked in LDS),
18944 (rounds of 40, three chunks per lane), 32768 (rounds of 64, four chunks), 64-wide groups at 5120 and 4544 (K % 128 == 64),
3 bits at 5120 and at 3584 with 64-wide groups; groups of one, two and three layers, the three-layer ones with N = (512, 256, 256) so
that blocks of the narrower members leave before the barrier, and once N = 8192 at K = 4096 (more strips than CUs).

Measured on an MI355X: rstd within 1.2e-7 relative of float64 in every cell (bounds 8e-6 .. 2e-3); the printed differ-shares are 0 in
188 of the 200 cells; in the eight fp16 cells at K = 3584 0.112 % of the xn elements of both kernels and 12-15 % of the outputs differ
from the eager path in their last bits, in the four fp16 cells at K = 6144 0.065 % of the standalone kernel's xn only -- DESIGN 3.11.

CASES holds one case for every NORM form of csrc/strip1_forms.hpp's table (MORE, below)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from gpu_util import Ref, guarded, randx, synth, to_layer
from test_swiglu_gpu import KINDS, SENTINEL, VARIANTS, _native, nw16_cases  # noqa: F401  (nw16_cases: the autouse fixture of the "+nw16" kinds)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.bfloat16)
EPS = 1e-5

# (kind, K, Ns, what the plan line must contain)
CASES = [("w4", 256, (256,), "nw=4 round=8 grid"), ("w4", 1024, (256, 256), "nw=4 round=8 exact"), ("w4", 3584, (2304, 2304), "nw=7 round=16 exact"),
         ("w4", 11008, (512, 256, 256), "nw=15 round=24 grid"), ("w4", 18944, (256, 256), "round=40 "), ("w4", 32768, (256,), "round=64 exact"),
         ("g64", 5120, (256, 256), " g64 "), ("g64", 4544, (256,), " g64 "), ("b3", 5120, (512, 256, 256), " bits=3 "), ("b3g64", 3584, (256, 256), " g64 bits=3 "),
         ("w4", 4096, (8192, 4096, 256), "nw=8 round=16 exact")]
IDS = [f"{k}-K{K}-x{len(ns)}" for k, K, ns, _ in CASES]
# One single-layer case for every NORM form of csrc/strip1_forms.hpp's table that the list above does not plan to (tests/test_swiglu_gpu.py,
# MORE: the same rule for N and K), in front of the last case.
MORE = [("b3", 256, (256,), "nw=4 round=8 bits=3 grid"), ("g64", 256, (256,), "nw=4 round=8 g64 grid"), ("b3g64", 256, (256,), "nw=4 round=8 g64 bits=3 grid"),
        ("b3", 1024, (256,), "nw=4 round=8 exact bits=3 grid"), ("g64", 1024, (256,), "nw=4 round=8 exact g64 grid"), ("b3g64", 1024, (256,), "nw=4 round=8 exact g64 bits=3 grid"),
        ("w4", 1152, (256,), "nw=4 round=16 grid"), ("b3", 1152, (256,), "nw=4 round=16 bits=3 grid"), ("g64", 1152, (256,), "nw=4 round=16 g64 grid"),
        ("b3g64", 1152, (256,), "nw=4 round=16 g64 bits=3 grid"), ("w4", 2048, (256,), "nw=4 round=16 exact grid"), ("b3", 2048, (256,), "nw=4 round=16 exact bits=3 grid"),
        ("g64", 2048, (256,), "nw=4 round=16 exact g64 grid"), ("b3g64", 2048, (256,), "nw=4 round=16 exact g64 bits=3 grid"), ("w4", 3584, (256,), "nw=4 round=32 grid"),
        ("b3", 3584, (256,), "nw=4 round=32 bits=3 grid"), ("g64", 3584, (256,), "nw=4 round=32 g64 grid"), ("w4", 4096, (256,), "nw=4 round=32 exact grid"),
        ("b3", 4096, (256,), "nw=4 round=32 exact bits=3 grid"), ("g64", 4096, (256,), "nw=4 round=32 exact g64 grid"), ("b3g64", 4096, (256,), "nw=4 round=32 exact g64 bits=3 grid"),
        ("w4", 3200, (8192,), "nw=7 round=16 grid"), ("b3", 3200, (8192,), "nw=7 round=16 bits=3 grid"), ("g64", 3200, (8192,), "nw=7 round=16 g64 grid"),
        ("b3g64", 3200, (8192,), "nw=7 round=16 g64 bits=3 grid"), ("b3", 3584, (8192,), "nw=7 round=16 exact bits=3 grid"), ("g64", 3584, (8192,), "nw=7 round=16 exact g64 grid"),
        ("b3g64", 3584, (8192,), "nw=7 round=16 exact g64 bits=3 grid"), ("w4", 3840, (8192,), "nw=8 round=16 grid"), ("b3", 3840, (8192,), "nw=8 round=16 bits=3 grid"),
        ("g64", 3840, (8192,), "nw=8 round=16 g64 grid"), ("b3g64", 3840, (8192,), "nw=8 round=16 g64 bits=3 grid"), ("b3", 4096, (8192,), "nw=8 round=16 exact bits=3 grid"),
        ("g64", 4096, (8192,), "nw=8 round=16 exact g64 grid"), ("b3g64", 4096, (8192,), "nw=8 round=16 exact g64 bits=3 grid"), ("w4", 5120, (256,), "nw=8 round=24 grid"),
        ("b3g64", 5120, (256,), "nw=8 round=24 g64 bits=3 grid"), ("w4", 6144, (256,), "nw=8 round=24 exact grid"), ("b3", 6144, (256,), "nw=8 round=24 exact bits=3 grid"),
        ("g64", 6144, (256,), "nw=8 round=24 exact g64 grid"), ("b3g64", 6144, (256,), "nw=8 round=24 exact g64 bits=3 grid"), ("w4", 6656, (256,), "nw=8 round=32 grid"),
        ("b3", 6656, (256,), "nw=8 round=32 bits=3 grid"), ("g64", 6656, (256,), "nw=8 round=32 g64 grid"), ("b3g64", 6656, (256,), "nw=8 round=32 g64 bits=3 grid"),
        ("w4", 8192, (256,), "nw=8 round=32 exact grid"), ("b3", 8192, (256,), "nw=8 round=32 exact bits=3 grid"), ("g64", 8192, (256,), "nw=8 round=32 exact g64 grid"),
        ("b3g64", 8192, (256,), "nw=8 round=32 exact g64 bits=3 grid"), ("b3", 11008, (256,), "nw=15 round=24 bits=3 grid"), ("g64", 11008, (256,), "nw=15 round=24 g64 grid"),
        ("b3g64", 11008, (256,), "nw=15 round=24 g64 bits=3 grid"), ("w4", 11520, (256,), "nw=15 round=24 exact grid"), ("b3", 11520, (256,), "nw=15 round=24 exact bits=3 grid"),
        ("g64", 11520, (256,), "nw=15 round=24 exact g64 grid"), ("b3g64", 11520, (256,), "nw=15 round=24 exact g64 bits=3 grid"), ("w4+nw16", 6656, (256,), "nw=16 round=16 grid"),
        ("b3+nw16", 6656, (256,), "nw=16 round=16 bits=3 grid"), ("g64+nw16", 6656, (256,), "nw=16 round=16 g64 grid"), ("b3g64+nw16", 6656, (256,), "nw=16 round=16 g64 bits=3 grid"),
        ("w4+nw16", 8192, (256,), "nw=16 round=16 exact grid"), ("b3+nw16", 8192, (256,), "nw=16 round=16 exact bits=3 grid"), ("g64+nw16", 8192, (256,), "nw=16 round=16 exact g64 grid"),
        ("b3g64+nw16", 8192, (256,), "nw=16 round=16 exact g64 bits=3 grid"), ("w4", 11776, (256,), "nw=16 round=24 grid"), ("b3", 11776, (256,), "nw=16 round=24 bits=3 grid"),
        ("g64", 11776, (256,), "nw=16 round=24 g64 grid"), ("b3g64", 11776, (256,), "nw=16 round=24 g64 bits=3 grid"), ("w4", 12288, (256,), "nw=16 round=24 exact grid"),
        ("b3", 12288, (256,), "nw=16 round=24 exact bits=3 grid"), ("g64", 12288, (256,), "nw=16 round=24 exact g64 grid"), ("b3g64", 12288, (256,), "nw=16 round=24 exact g64 bits=3 grid"),
        ("w4", 14336, (256,), "nw=16 round=32 grid"), ("b3", 14336, (256,), "nw=16 round=32 bits=3 grid"), ("g64", 14336, (256,), "nw=16 round=32 g64 grid"),
        ("b3g64", 14336, (256,), "nw=16 round=32 g64 bits=3 grid"), ("w4", 16384, (256,), "nw=16 round=32 exact grid"), ("b3", 16384, (256,), "nw=16 round=32 exact bits=3 grid"),
        ("g64", 16384, (256,), "nw=16 round=32 exact g64 grid"), ("b3g64", 16384, (256,), "nw=16 round=32 exact g64 bits=3 grid"), ("g64", 18944, (256,), "nw=16 round=40 g64 grid"),
        ("w4", 20480, (256,), "nw=16 round=40 exact grid"), ("g64", 20480, (256,), "nw=16 round=40 exact g64 grid"), ("w4", 22016, (256,), "nw=16 round=48 grid"),
        ("g64", 22016, (256,), "nw=16 round=48 g64 grid"), ("w4", 24576, (256,), "nw=16 round=48 exact grid"), ("g64", 24576, (256,), "nw=16 round=48 exact g64 grid"),
        ("w4", 26624, (256,), "nw=16 round=56 grid"), ("w4", 28672, (256,), "nw=16 round=56 exact grid"), ("w4", 28800, (256,), "nw=16 round=64 grid")]
CASES[-1:-1] = MORE
IDS[-1:-1] = [f"{k}-K{K}-N{ns[0]}" for k, K, ns, _ in MORE]
BIG = CASES[-1]


@functools.lru_cache(maxsize=None)
def _group(kind, K, Ns, variant=None, compat=0):
    """[(synth dict, q_layer, native descriptor, keepalive)] of one sibling group: built once per case and shared by the tests below.  Zero
    points / bias / layout rotate over the cases as VARIANTS does in tests/test_swiglu_gpu.py (one variant per group: the members of a
    grouped launch share their layout family)."""
    bits, g = KINDS[kind]
    idx = [c[:3] for c in CASES].index((kind, K, Ns)) if variant is None else variant
    layout, zk, bias = VARIANTS[idx % len(VARIANTS)]
    out = []
    for i, N in enumerate(Ns):
        d = synth(layout, bits, g, K, N, zk, False, bias, seed=K + N + g + bits + 31 * i)
        d["scales"] = (d["scales"].astype(np.float32) * (4096 / K) ** 0.5 * 0.5).astype(np.float16)
        d["compat"] = compat
        layer = to_layer(d, DEV)
        w, keep = _native(layer, d, zk, compat)
        out.append((d, layer, w, keep))
    return tuple(out)


def _descs(group):
    return [m[2] for m in group]


def _wnorm(K, dtype, seed=0):
    return torch.from_numpy((np.random.default_rng(seed + K).standard_normal(K) * 0.2 + 1.0).astype(np.float32)).to(dtype).to(DEV)


def _x(K, dtype, seed=1, kind="randx"):
    x = randx(1, K, seed=seed).astype(np.float32)
    if kind == "massive":   # a massive-activation row: eight entries at +-2000
        at = np.random.default_rng(seed).choice(K, 8, replace=False)
        x[0, at] = 2000.0 * np.sign(x[0, at])
    if kind == "zero":
        x[:] = 0
    return torch.from_numpy(x).to(dtype).to(DEV)


def _xn(x, w_norm, rstd):
    return w_norm * (x.float() * rstd[:, None]).to(x.dtype)


def _eager(x, w_norm, eps=EPS):
    """transformers' LlamaRMSNorm.forward, expression for expression."""
    h = x.to(torch.float32)
    var = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(var + eps)
    return w_norm * h.to(x.dtype)


def _rstd64(x, eps=EPS):
    x64 = x.double()
    return 1.0 / torch.sqrt((x64 * x64).mean(-1) + eps)


def _check_plan(descs, tag=None):
    from qllm_amd import ops
    plan = ops.plan_describe(descs, 1)
    assert plan.startswith("strip1 "), plan
    assert ops.rmsnorm_describe(descs, 1) == "rmsnorm " + plan
    if tag is not None:
        assert tag in plan + " ", (tag, plan)
    return plan


# ---- rstd ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,Ns,tag", CASES[:-1], ids=IDS[:-1])
def test_rstd_of_the_fused_entry_matches_float64(kind, K, Ns, tag):
    from qllm_amd import ops
    descs = _descs(_group(kind, K, Ns))
    bound = (K / 2 + 8) * 2.0 ** -24
    for dtype in DTYPES:
        w_norm = _wnorm(K, dtype)
        for xk in ("randx", "massive", "zero"):
            x = _x(K, dtype, seed=K % 97, kind=xk)
            outs, rstd = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS, return_rstd=True)
            want = _rstd64(x)
            rel = float(((rstd.double() - want).abs() / want).max())
            print(f"\nrstd fused kind={kind} K={K} {str(dtype)[6:]} {xk}: rel={rel:.3e} bound={bound:.3e}", end="")
            assert rel <= bound, (kind, K, dtype, xk, rel, bound)
            assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
            if xk == "zero":
                assert abs(float(rstd[0]) - EPS ** -0.5) <= bound * EPS ** -0.5


@pytest.mark.parametrize("K", [256, 4544, 11008, 32768, 65536])
def test_rstd_of_the_standalone_kernel_matches_float64(K):
    from qllm_amd import ops
    bound = (K / 2 + 8) * 2.0 ** -24
    for dtype in DTYPES:
        w_norm = _wnorm(K, dtype)
        x = torch.cat([_x(K, dtype, seed=3), _x(K, dtype, seed=4, kind="massive"), _x(K, dtype, kind="zero")])
        y, rstd = ops.rmsnorm(x, w_norm, EPS, return_rstd=True)
        want = _rstd64(x)
        rel = float(((rstd.double() - want).abs() / want).max())
        print(f"\nrstd standalone K={K} {str(dtype)[6:]}: rel={rel:.3e} bound={bound:.3e}", end="")
        assert rel <= bound, (K, dtype, rel, bound)
        assert bool(torch.isfinite(y.float()).all()) and bool((y[2] == 0).all())


# ---- bit identity of the staging ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,Ns,tag", CASES, ids=IDS)
def test_bit_identity_with_the_plain_grouped_launch(kind, K, Ns, tag):
    """linear_forward_rmsnorm(descs, x, w, eps) == linear_forward_grouped(descs, w * (x.float() * rstd).to(dtype)) on every member, with
    rstd the launch's own report: pins the staging -- windows, xkeep, the shifted last window, the parked weight chunks, the odd wave
    counts, 1..4 chunks per lane -- and, the plain launch being fed ONE rstd, that every block of the fused launch used that very value
    (at N = (8192, 4096, 256), K = 4096: 784 blocks on three siblings, more than the CUs; a block with another rstd fails here)."""
    from qllm_amd import ops
    descs = _descs(_group(kind, K, Ns))
    _check_plan(descs, tag)
    for dtype in DTYPES:
        w_norm = _wnorm(K, dtype, seed=5)
        for xk in ("randx", "massive"):
            x = _x(K, dtype, seed=K % 89 + 2, kind=xk)
            fused, rstd = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS, return_rstd=True)
            xn = _xn(x, w_norm, rstd)
            assert xn.dtype == dtype and bool(torch.isfinite(xn.float()).all())
            plain = ops.linear_forward_grouped(descs, xn)
            for i, (f, p) in enumerate(zip(fused, plain)):
                assert f.dtype == dtype and f.shape == (1, Ns[i])
                assert torch.equal(f, p), (kind, K, Ns, i, dtype, xk, int((f != p).sum()))


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_zero_kinds_bias_and_the_autogptq_offset(variant):
    """Packed, fp16 and symmetric zero points, with and without bias, on the K = 11008 form with three members, and the AutoGPTQ offset on
    the packed case."""
    from qllm_amd import ops
    K, Ns = 11008, (512, 256, 256)
    layout, zk, _ = VARIANTS[variant]
    for compat in ((0, 1) if (layout, zk) == ("GPTQ", "asym") else (0,)):
        group = _group("w4", K, Ns, variant, compat)
        descs = _descs(group)
        assert all(w.add_zero_bias == compat for w in descs)
        for dtype in DTYPES:
            w_norm, x = _wnorm(K, dtype, seed=variant), _x(K, dtype, seed=variant + 20)
            fused, rstd = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS, return_rstd=True)
            for f, p in zip(fused, ops.linear_forward_grouped(descs, _xn(x, w_norm, rstd))):
                assert torch.equal(f, p), (variant, compat, dtype)
        if compat:   # the offset is really applied: against the oracle with compat = 1
            x, w_norm = _x(K, torch.float16, seed=9), _wnorm(K, torch.float16)
            y = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS)[0]
            assert O.rel_err(y.cpu().numpy(), Ref(group[0][0]).y16(_eager(x, w_norm).cpu().numpy())) <= 1e-2


@pytest.mark.parametrize("K", [256, 4544, 11008, 32768])
def test_standalone_kernel_bit_identity(K):
    """ops.rmsnorm: y == w * (x.float() * rstd).to(dtype) bit for bit with its own rstd, at 1, 3 and 130 rows."""
    from qllm_amd import ops
    for dtype in DTYPES:
        w_norm = _wnorm(K, dtype, seed=2)
        for m in (1, 3, 130):
            x = torch.from_numpy(randx(m, K, seed=K % 83 + m)).to(dtype).to(DEV)
            if m == 3:
                x[1, ::K // 8] *= 1500
            y, rstd = ops.rmsnorm(x, w_norm, EPS, return_rstd=True)
            assert y.shape == x.shape and y.dtype == dtype and rstd.shape == (m,)
            assert torch.equal(y, _xn(x, w_norm, rstd)), (K, m, dtype)
            assert torch.equal(ops.rmsnorm(x.view(1, m, K), w_norm, EPS).view(m, K), y)   # leading dimensions are rows


# ---- against eager and the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,Ns,tag", CASES[:-1], ids=IDS[:-1])
def test_against_the_eager_norm_and_the_oracle(kind, K, Ns, tag, capsys):
    """The fused launch against the eager transformers expression followed by the plain grouped launch: the oracle's fp16 result and float64
    on the eager xn, with the tolerances of tests/test_strip1_gpu.py.  Prints the share of outputs (and of xn elements, for both kernels)
    whose bits differ from the eager path."""
    from qllm_amd import ops
    group = _group(kind, K, Ns)
    descs = _descs(group)
    ref = Ref(group[0][0])
    for dtype in DTYPES:
        w_norm, x = _wnorm(K, dtype, seed=7), _x(K, dtype, seed=K % 79 + 5)
        xe = _eager(x, w_norm)
        fused, rstd = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS, return_rstd=True)
        plain = ops.linear_forward_grouped(descs, xe)
        differ = float(torch.cat([(f != p).float().flatten() for f, p in zip(fused, plain)]).mean())
        xn_f = float((_xn(x, w_norm, rstd) != xe).float().mean())
        xn_s = float((ops.rmsnorm(x, w_norm, EPS) != xe).float().mean())
        with capsys.disabled():
            print(f"\nrmsnorm differ-share kind={kind} K={K} {str(dtype)[6:]}: y={differ:.5f} xn_fused={xn_f:.5f} xn_standalone={xn_s:.5f}", end="")
        xn = xe.float().cpu().numpy().astype(np.float16)   # (bf16: the kernel stages fp16 -- what test_strip1_gpu.py compares with)
        yn = fused[0].float().cpu().numpy()
        assert np.isfinite(yn).all()
        e16 = O.rel_err(yn, ref.y16(xn))
        e64 = O.rel_err(yn.astype(np.float64), ref.y64(xn))
        assert e16 <= 1e-2, (kind, K, dtype, e16)
        assert e64 <= (2e-3 if dtype == torch.float16 else 2e-2), (kind, K, dtype, e64)


# ---- memory -------------------------------------------------------------------------------------------------------------------------------
def _carve_out(m, n, dtype, band=2048):
    buf = torch.full((band + m * n + band,), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf[band:band + m * n].view(dtype).view(m, n), band


def _carve_rstd(m, band=64):
    buf = torch.full((band + m + band,), -7.5, dtype=torch.float32, device=DEV)
    return buf, buf[band:band + m], band


GUARD = [c for c in CASES if (c[0], c[1]) in (("w4", 256), ("w4", 11008), ("w4", 32768), ("g64", 5120), ("b3", 5120))]


@pytest.mark.parametrize("kind,K,Ns,tag", GUARD, ids=[f"{c[0]}-K{c[1]}" for c in GUARD])
def test_reads_and_writes_stay_inside_their_tensors(kind, K, Ns, tag):
    """x, w_norm, every y and rstd_out carved out of larger buffers: NaN bands around the inputs, sentinel bands around the outputs.  A
    read outside x or w_norm puts a NaN into rstd or the outputs; a store outside an output changes a band.  Both entries; the standalone
    kernel also in place."""
    from qllm_amd import ops
    descs = _descs(_group(kind, K, Ns))
    for dtype in DTYPES:
        x0, w0 = _x(K, dtype, seed=11), _wnorm(K, dtype, seed=11)
        xbuf, x = guarded(x0)
        wbuf, w_norm = guarded(w0)
        ys = [_carve_out(1, n, dtype) for n in Ns]
        rbuf, r, rband = _carve_rstd(1)
        outs, rstd = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS, outs=[y[1] for y in ys], return_rstd=r)
        torch.cuda.synchronize()
        assert rstd.data_ptr() == r.data_ptr() and bool(torch.isfinite(r).all())
        assert bool((rbuf[:rband] == -7.5).all()) and bool((rbuf[rband + 1:] == -7.5).all()), "a store outside rstd_out"
        for (ybuf, y, band), n in zip(ys, Ns):
            assert bool(torch.isfinite(y.float()).all()), (kind, K, dtype)
            assert bool((ybuf[:band] == SENTINEL).all()) and bool((ybuf[band + n:] == SENTINEL).all()), "a store outside y"
        for buf, view, orig in ((xbuf, x, x0), (wbuf, w_norm, w0)):
            lead = (buf.numel() - K) // 2
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + K:]).all())
            assert torch.equal(view, orig)
        for y, want in zip(outs, ops.linear_forward_rmsnorm(descs, x0, w0, EPS)):
            assert torch.equal(y, want)
        # the standalone kernel: three rows, out of place into a carved y, then in place
        m = 3
        x3 = torch.from_numpy(randx(m, K, seed=12)).to(dtype).to(DEV)
        xbuf, x = guarded(x3)
        ybuf, y, band = _carve_out(m, K, dtype)
        rbuf, r, rband = _carve_rstd(m)
        ops.rmsnorm(x, w_norm, EPS, out=y, return_rstd=r)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(r).all())
        assert bool((ybuf[:band] == SENTINEL).all()) and bool((ybuf[band + m * K:] == SENTINEL).all())
        assert bool((rbuf[:rband] == -7.5).all()) and bool((rbuf[rband + m:] == -7.5).all())
        assert torch.equal(x, x3) and torch.equal(w_norm, w0)
        want = y.clone()
        assert ops.rmsnorm(x, w_norm, EPS, out=x) is x      # in place
        torch.cuda.synchronize()
        lead = (xbuf.numel() - m * K) // 2
        assert torch.equal(x, want) and bool(torch.isnan(xbuf[:lead]).all()) and bool(torch.isnan(xbuf[lead + m * K:]).all())


# ---- determinism, capture, refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,Ns,tag", [CASES[3], CASES[6], CASES[8]], ids=[IDS[3], IDS[6], IDS[8]])
def test_deterministic_and_capturable(kind, K, Ns, tag):
    """Two calls give the same bits; both entries captured on one stream (no parallel branches) and replayed twice equal the eager calls."""
    from qllm_amd import ops
    descs = _descs(_group(kind, K, Ns))
    x, w_norm = _x(K, torch.float16, seed=21), _wnorm(K, torch.float16, seed=21)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [o.clone() for o in ops.linear_forward_rmsnorm(descs, x, w_norm, EPS)]
        again = [o.clone() for o in ops.linear_forward_rmsnorm(descs, x, w_norm, EPS)]
        alone = ops.rmsnorm(x, w_norm, EPS).clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = ops.linear_forward_rmsnorm(descs, x, w_norm, EPS)
        yn = ops.rmsnorm(x, w_norm, EPS)
    for _ in range(2):
        for y in ys + [yn]:
            y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ys, eager)) and torch.equal(yn, alone)


def test_refusals_on_the_device():
    """What the fused entry does not serve raises QllmUnsupported and leaves y and rstd_out alone: two rows, a reference-layout descriptor,
    4 bits with 32-wide groups."""
    from qllm_amd import ops
    group = _group("w4", 1024, (256, 256))
    d32 = synth("GPTQ", 4, 32, 1024, 256, "asym", False, False, seed=3)
    l32 = to_layer(d32, DEV)
    w32 = l32.native_descriptor(0) or l32._descriptor(None, 0)
    for descs, m in ((_descs(group), 2), ([group[0][1]._descriptor(None, 0)] * 2, 1), ([w32], 1)):
        x = torch.ones((m, 1024), dtype=torch.float16, device=DEV)
        ys = [torch.full((m, 256), 3.0, dtype=torch.float16, device=DEV) for _ in descs]
        r = torch.full((m,), -7.5, dtype=torch.float32, device=DEV)
        assert ops.rmsnorm_describe(descs, m).startswith("refused: ")
        with pytest.raises(ops.QllmUnsupported):
            ops.linear_forward_rmsnorm(descs, x, _wnorm(1024, torch.float16), EPS, outs=ys, return_rstd=r)
        torch.cuda.synchronize()
        assert all(bool((y == 3.0).all()) for y in ys) and bool((r == -7.5).all())


# ---- module level -------------------------------------------------------------------------------------------------------------------------
def _tiny_layer(layout, g):
    """A LlamaDecoderLayer of quantized linears (hidden 256, intermediate 512): transformers' own classes, its norms with random weights."""
    import transformers
    from transformers.models.llama import modeling_llama as ML
    from qllm_amd.modeling.q_layers import install_sibling_groups
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
                                   vocab_size=32, rms_norm_eps=EPS)
    cfg._attn_implementation = "eager"
    layer = ML.LlamaDecoderLayer(cfg, 0).half()
    shapes = {"q_proj": (256, 256), "k_proj": (256, 256), "v_proj": (256, 256), "o_proj": (256, 256)}
    for i, (name, (K, N)) in enumerate(shapes.items()):
        d = synth(layout, 4, g, K, N, "asym", False, False, seed=60 + i + g)
        d["scales"] = (d["scales"].astype(np.float32) * 0.25).astype(np.float16)
        setattr(layer.self_attn, name, to_layer(d, DEV))
    for i, (name, K, N) in enumerate((("gate_proj", 256, 512), ("up_proj", 256, 512), ("down_proj", 512, 256))):
        d = synth(layout, 4, g, K, N, "asym", False, False, seed=70 + i + g)
        d["scales"] = (d["scales"].astype(np.float32) * 0.25).astype(np.float16)
        setattr(layer.mlp, name, to_layer(d, DEV))
    gen = torch.Generator().manual_seed(g)
    for norm in (layer.input_layernorm, layer.post_attention_layernorm):
        norm.weight.data = (torch.randn(256, generator=gen) * 0.2 + 1).half()
    layer = layer.to(DEV).eval()
    assert install_sibling_groups(layer, [type(layer.mlp.down_proj)]) == 2
    rope = ML.LlamaRotaryEmbedding(cfg).to(DEV)
    return layer, rope


def _run(layer, rope, x):
    m = x.shape[1]
    pos = torch.arange(m, device=DEV)[None]
    mask = torch.full((m, m), float("-inf"), device=DEV, dtype=x.dtype).triu(1)[None, None]
    out = layer(x, attention_mask=mask, position_ids=pos, position_embeddings=rope(x, pos))
    return out[0] if isinstance(out, tuple) else out


@pytest.mark.parametrize("layout,g", [("GPTQ", 128), ("HQQ", 64)])
def test_decoder_layer_with_the_fused_norms(layout, g):
    from qllm_amd.modeling.q_layers import fused_norm, install_fused_norm, uninstall_fused_norm
    layer, rope = _tiny_layer(layout, g)
    q_type = type(layer.mlp.down_proj)
    xs = {m: torch.from_numpy(randx(m, 256, seed=m)).to(DEV).view(1, m, 256) for m in (1, 2, 40)}
    with torch.no_grad():
        before = {m: _run(layer, rope, x.clone()) for m, x in xs.items()}
        assert install_fused_norm(layer, [q_type]) == 2
        groups = (layer.self_attn.q_proj._siblings, layer.mlp.gate_proj._siblings)
        pres = [layer.self_attn.q_proj.__dict__[fused_norm._PRENORM][0], layer.mlp.up_proj.__dict__[fused_norm._PRENORM][0]]
        for m, x in xs.items():
            n0 = [gr.grouped_launches for gr in groups]
            f0 = [p.fused_launches for p in pres]
            after = _run(layer, rope, x.clone())
            a, b = after.float().cpu().numpy().reshape(m, -1), before[m].float().cpu().numpy().reshape(m, -1)
            e16, e64 = O.rel_err(a, b), O.rel_err(a.astype(np.float64), b.astype(np.float64))
            print(f"\nlayer {layout} g{g} rows={m}: rel_err={e16:.2e}", end="")
            assert e16 <= 1e-2 and e64 <= 2e-3, (m, e16, e64)
            if m == 1:
                assert [gr.grouped_launches - n for gr, n in zip(groups, n0)] == [1, 1]  # one grouped launch per norm
            assert [p.fused_launches - f for p, f in zip(pres, f0)] == ([1, 1] if m <= fused_norm.PreNorm.norm_max_m else [0, 0])
            assert not any(gr._parked for gr in groups) and not any(p.refused for p in pres)   # the parked outputs were consumed
        fused_norm.PreNorm.norm_max_m, keep = 1, fused_norm.PreNorm.norm_max_m           # the fused entry, whatever the modules' default
        try:
            f0 = [p.fused_launches for p in pres]
            after = _run(layer, rope, xs[1].clone())
            assert [p.fused_launches - f for p, f in zip(pres, f0)] == [1, 1]
            a, b = after.float().cpu().numpy().reshape(1, -1), before[1].float().cpu().numpy().reshape(1, -1)
            assert O.rel_err(a, b) <= 1e-2 and O.rel_err(a.astype(np.float64), b.astype(np.float64)) <= 2e-3
        finally:
            fused_norm.PreNorm.norm_max_m = keep
        assert uninstall_fused_norm(layer) == 2
        for m, x in xs.items():
            assert torch.equal(_run(layer, rope, x.clone()), before[m]), m


def test_load_quantized_with_fuse_norm_generates_the_same_tokens(tmp_path):
    """load_quantized(fuse_norm=True, fuse_mlp=True) against fuse_norm=False on a saved tiny checkpoint: 8 greedy steps with a KV cache
    (one row per step), both models fed the plain model's tokens.  Where the argmax differs the test reports the plain model's logit margin
    between the two tokens and fails only above the tolerance-implied bound: both logit vectors are within rel_err 2e-2 (the loader
    test's bound, tests/test_swiglu_gpu.py) of each other, i.e. within 2e-2 * max|logit| per element, so two tokens can swap only if their
    margin is at most twice that."""
    from test_loader_repack_cpu import _quantize_in_place, _tiny_llama
    from qllm_amd.modeling import base
    model, names = _quantize_in_place(_tiny_llama(), "GPTQ")
    d = str(tmp_path / "ckpt")
    base.save_quantized(model, d)
    plain = base.load_quantized(d, device=DEV)
    assert not hasattr(plain, "fused_norms")                      # off by default
    fused = base.load_quantized(d, device=DEV, fuse_norm=True, fuse_mlp=True)
    assert fused.fused_norms == 4 and fused.quant_norms == 1 and fused.fused_mlps == 2
    tok = torch.tensor([[5]], device=DEV)
    pkv_p = pkv_f = None
    with torch.no_grad():
        for step in range(8):
            op = plain(tok, past_key_values=pkv_p, use_cache=True)
            of = fused(tok, past_key_values=pkv_f, use_cache=True)
            pkv_p, pkv_f = op.past_key_values, of.past_key_values
            lp, lf = op.logits[0, -1].float(), of.logits[0, -1].float()
            assert O.rel_err(lf.cpu().numpy()[None], lp.cpu().numpy()[None]) <= 2e-2, step
            tp, tf = int(lp.argmax()), int(lf.argmax())
            if tp != tf:
                margin, bound = float(lp[tp] - lp[tf]), 2 * 2e-2 * float(lp.abs().max())
                print(f"\nstep {step}: tokens {tp} / {tf}, margin {margin:.4e}, bound {bound:.4e}", end="")
                assert margin <= bound, (step, tp, tf, margin, bound)
            tok = torch.tensor([[tp]], device=DEV)
