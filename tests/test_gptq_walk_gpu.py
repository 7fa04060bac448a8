"""-m gpu: qllm_gptq_quantize (csrc/gptq_quant.hip) and qllm_gptq_quantize_static (csrc/gptq_static.hip) bit for bit against the float32
walk of tests/gptq_walk_cases.py, over that module's case matrix: codes, the scale and zero of every group, wq (the walk's value rounded
once to the storage type: the float32 cases see every bit), the loss of every row, and the workspace (Err[N][K] in processing order for
every block but the last; every other byte as the test left it).  The walk itself is checked in tests/test_gptq_walk_cpu.py.

Nothing is compared with a tolerance and no case of the matrix is left out.  Case count and time: profiles/gptq_quantize.md."""
import numpy as np
import pytest
import torch

import gptq_walk_cases as C
from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
NAMES = ("codes", "scale", "zero", "wq", "loss")


def bits_of(t):
    return t.contiguous().view(BITS.get(t.dtype, t.dtype))


def kernel(c, W, U, perm, rows=None):
    """The case's entry point on W [N, K] float32 numpy (`rows`: on those rows only) with the test's own outputs and a 0xFF-filled
    workspace of exactly the size the library asks for: ((codes [N, K] as the kernel orders its columns, scale, zero, wq, loss), workspace)."""
    dt = C.DTYPES[c["dtype"]]
    Wd = torch.from_numpy(W if rows is None else W[rows]).to(dt).to(DEV).contiguous()
    assert torch.equal(Wd.float().cpu(), torch.from_numpy(W if rows is None else W[rows]))       # exactly representable
    N, K, G = Wd.shape[0], c["K"], c["K"] // c["g"]
    Ud = None if U is None else torch.from_numpy(U).to(DEV)
    out = (torch.full((K, N), -77, dtype=torch.int32, device=DEV), torch.full((N, G), float("nan"), device=DEV),
           torch.full((N, G), float("nan"), device=DEV), torch.full((N, K), float("nan"), dtype=dt, device=DEV),
           torch.full((N,), float("nan"), device=DEV))
    need = ops._lib.load().qllm_gptq_quantize_workspace_bytes(N, K)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    if c["kernel"] == "static":
        ops.gptq_quantize_static(Wd, Ud, None if perm is None else torch.from_numpy(perm).to(DEV), c["bits"], c["g"], bool(c["sym"]), out=out,
                                 workspace=ws)
    else:
        ops.gptq_quantize(Wd, Ud, c["bits"], c["g"], bool(c["sym"]), out=out, workspace=ws)
    torch.cuda.synchronize()
    return (out[0].t().contiguous().cpu(),) + tuple(t.cpu() for t in out[1:]), ws.cpu()


def check(c):
    W, U, perm = C.inputs(c)
    codes, scale, zero, dq, err, loss = C.run(c)
    dt, N, K = C.DTYPES[c["dtype"]], c["N"], c["K"]
    got, ws = kernel(c, W, U, perm)
    want = (torch.from_numpy(codes), torch.from_numpy(scale), torch.from_numpy(zero), torch.from_numpy(dq).to(dt), torch.from_numpy(loss))
    for name, a, b in zip(NAMES, got, want):
        differ = bits_of(a) != bits_of(b)
        assert not bool(differ.any()), f"{c['id']}: {name}: {int(differ.sum())} of {differ.numel()} differ, first at {differ.nonzero()[0].tolist()}"
    # the workspace: the errors of every block but the last, by processing position; nothing else was written
    kept = 0 if U is None else (K - 1) // C.BLK * C.BLK
    history = ws[:N * K * 4].view(torch.int32).view(N, K)
    differ = history[:, :kept] != torch.from_numpy(err[:, :kept].copy()).view(torch.int32)
    assert not bool(differ.any()), f"{c['id']}: err: {int(differ.sum())} differ, first at (row, position) {differ.nonzero()[0].tolist()}"
    assert bool((history[:, kept:] == -1).all()) and bool((ws[N * K * 4:] == 0xFF).all()), c["id"]


def chunks(cases, n):
    return [pytest.param(cases[i:i + n], id=f"{cases[i]['kernel']}{i // n}") for i in range(0, len(cases), n)]


@pytest.mark.parametrize("cases", chunks(C.DYNAMIC, 8))
def test_dynamic_kernel_equals_the_walk_bit_for_bit(cases):
    for c in cases:
        check(c)


@pytest.mark.parametrize("cases", chunks(C.STATIC, 8))
def test_static_kernel_equals_the_walk_bit_for_bit(cases):
    for c in cases:
        check(c)


@pytest.mark.parametrize("cid", ["dyn-N40-K320-g64-w4a-float16-randn-dense", "static-N40-K416-g32-w4a-float16-randn-dense-random",
                                 "static-N40-K1024-g64-w4a-float16-randn-dense-random"])
def test_rows_of_a_ragged_tile_quantized_alone_give_the_same_bits(cid):
    """N = 40: two full row tiles and one of 8 rows.  Rows are independent, so rows of each tile, quantized alone in other lanes of another
    tile, give what they gave in place (both kernels)."""
    c = C.BY_ID[cid]
    W, U, perm = C.inputs(c)
    rows = np.array([0, 15, 16, 31, 32, 39])
    full, _ = kernel(c, W, U, perm)
    part, _ = kernel(c, W, U, perm, rows)
    for name, a, b in zip(NAMES, full, part):
        assert torch.equal(bits_of(a[rows]), bits_of(b)), name
