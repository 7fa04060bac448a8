"""The routed-experts entries above four tokens without a device (qllm_moe_route, qllm_moe_prefill_gate_up, qllm_moe_prefill_down,
qllm_moe_prefill_workspace_bytes, qllm_moe_prefill_describe; csrc/moe_prefill.hip): the symbols, every refusal of the C entries -- reached
with fake pointers, before any device work --, the workspace's size, ops.moe_prefill_plan's reasons and the kernels' resources."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from kernel_resources import resources
from test_moe_decode_cpu import _plan_args, _stack
from qllm_amd import _lib, ops

ENTRIES = ("qllm_moe_route", "qllm_moe_prefill_gate_up", "qllm_moe_prefill_down", "qllm_moe_prefill_describe", "qllm_moe_prefill_workspace_bytes")
INVALID, UNSUPPORTED = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED
P = lambda n: n << 20   # noqa: E731  fake pointers: aligned, distinct, never dereferenced
GOOD = dict(T=5, top_k=2, E=8, H=256, I=384, tile=0, azb=0, dt=_lib.DT_F16, wdt=_lib.DT_F32, x=P(1), ids=P(2), wts=P(3), ws=P(4), nws=1 << 30, qw=P(5), sc=P(6),
            qz=P(7), qz2=P(7), out=P(8))
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: only where no HIP device is visible")


def _call(entry, **change):
    a = dict(GOOD, **change)
    lib, sizes = _lib.load(), (a["T"], a["top_k"], a["E"], a["H"], a["I"], a["tile"])
    if entry == "qllm_moe_route":
        rc = lib.qllm_moe_route(a["ids"], a["ws"], a["nws"], a["T"], a["top_k"], a["E"], a["tile"], None)
    elif entry == "qllm_moe_prefill_gate_up":
        rc = lib.qllm_moe_prefill_gate_up(a["x"], a["ws"], a["nws"], a["qw"], a["sc"], a["qz"], a["qw"], a["sc"], a["qz2"], a["out"], *sizes, a["azb"], a["dt"], None)
    elif entry == "qllm_moe_prefill_down":
        rc = lib.qllm_moe_prefill_down(a["x"], a["ids"], a["wts"], a["ws"], a["nws"], a["qw"], a["sc"], a["qz"], a["out"], *sizes, a["azb"], a["wdt"], a["dt"], None)
    else:
        buf = C.create_string_buffer(512)
        rc = lib.qllm_moe_prefill_describe(*sizes, buf, 512)
        return rc, buf.value.decode() if rc == 0 else _lib.last_error()
    return rc, _lib.last_error()


def test_symbols_options_and_describe_lines():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qllm_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b(int|size_t) {name}\(", header) and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert "#define QLLM_ABI_VERSION 7" in header
    assert {"moe_route", "moe_prefill_gate_up", "moe_prefill_down", "moe_prefill_plan", "moe_prefill_describe"} <= set(ops.__all__)
    from qllm_amd.modeling.base import load_quantized
    assert inspect.signature(load_quantized).parameters["fuse_moe_prefill"].default is False
    assert ops.moe_prefill_describe(16, 8, 128, 2048, 768).startswith("moe_prefill tile_rows=16 route grid=1 waves=16 lds=9280 | gate_up grid=136x12 waves=4 lds=16896 |")
    assert ops.moe_prefill_describe(2048, 2, 8, 4096, 14336).endswith("| down grid=72x32 waves=4 lds=67584 | combine grid=2x2048")
    assert ops.moe_prefill_describe(40000, 2, 8, 4096, 14336).startswith("refused: ") and ops.moe_describe(5, 2, 8, 256, 384).startswith("refused: ")


REFUSALS = [  # (entries: Route, Gate/up, Down, descrIbe), the change, status, a word of the message)
    ("G", dict(x=None), INVALID, "NULL"), ("D", dict(x=None), INVALID, "NULL"), ("RD", dict(ids=None), INVALID, "NULL"), ("GD", dict(out=None), INVALID, "NULL"),
    ("D", dict(wts=None), INVALID, "NULL"), ("RGD", dict(ws=None), INVALID, "NULL"), ("GD", dict(qw=None), INVALID, "NULL"), ("GD", dict(sc=None), INVALID, "NULL"),
    ("G", dict(qz2=None), INVALID, "both"), ("GD", dict(x=P(1) + 8), INVALID, "aligned"), ("RD", dict(ids=P(2) + 4), INVALID, "aligned"),
    ("RGD", dict(ws=P(4) + 128), INVALID, "aligned"), ("GD", dict(azb=2), INVALID, "add_zero_bias"), ("GD", dict(dt=_lib.DT_F32), INVALID, "act_dtype"),
    ("D", dict(wdt=_lib.DT_BF16), INVALID, "weights_dtype"), ("RGDI", dict(T=0), INVALID, ">= 1"), ("RGDI", dict(tile=32), INVALID, "tile_rows"),
    ("RGD", dict(nws=1024), INVALID, "too small"), ("D", dict(nws=2304), INVALID, "too small"),   # (2304: the table alone, without the product rows)
    ("RGDI", dict(T=32769), UNSUPPORTED, "slots"), ("RGDI", dict(E=1025), UNSUPPORTED, "experts"),
    ("RGDI", dict(top_k=9), UNSUPPORTED, "top_k"), ("GDI", dict(H=192), UNSUPPORTED, "128"), ("GDI", dict(I=320), UNSUPPORTED, "128"),
]


@no_device
@pytest.mark.parametrize("which,change,status,word", REFUSALS, ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_every_refusal_is_reached_before_any_device_work(which, change, status, word):
    for letter, entry in zip("RGDI", ENTRIES):
        if letter not in which:
            continue
        rc, text = _call(entry, **change)
        if letter == "I" and status == UNSUPPORTED:      # a describe entry answers a refusal as text
            assert rc == 0 and text.startswith("refused: ") and word in text, (rc, text)
        else:
            assert rc == status and word in text, (entry, rc, text)


def test_workspace_bytes_is_pure_grows_with_t_and_covers_both_tile_bounds():
    for top_k, e, h, i in ((2, 8, 4096, 14336), (8, 128, 2048, 768), (1, 1024, 128, 128)):
        sizes = [ops.moe_prefill_workspace_bytes(t, top_k, e, h, i) for t in (1, 5, 17, 70, 2048)]
        assert sizes == [ops.moe_prefill_workspace_bytes(t, top_k, e, h, i) for t in (1, 5, 17, 70, 2048)] and sizes == sorted(set(sizes))
        for t, size in zip((1, 5, 17, 70, 2048), sizes):
            s = t * top_k
            tiles = max(s // bm + min(e, s) for bm in (16, 64))
            rows = max((s // bm + min(e, s)) * bm for bm in (16, 64))
            assert size >= 4 * (16 + e + 2 * tiles + rows) + s * h * 2   # header, counts, two ints per tile, the padded rows; the product rows
    assert ops.moe_prefill_workspace_bytes(5, 9, 8, 256, 384) == 0 and ops.moe_prefill_workspace_bytes(5, 2, 8, 192, 384) == 0


def test_plan_serves_prompts_and_picks_the_tile_from_slots_per_expert():
    assert ops.moe_prefill_plan(*_plan_args(t=5)) == (5, 2, 4, 256, 384, 16)
    assert ops.moe_prefill_plan(*_plan_args(t=64, top_k=2, e=4, dtype=torch.bfloat16, wdtype=torch.bfloat16)) == (64, 2, 4, 256, 384, 64)
    assert ops.moe_prefill_plan(*_plan_args(t=64), tile_rows=16)[5] == 16 and ops.moe_prefill_plan(*_plan_args(t=4, top_k=2, e=8))[0] == 4


PLAN_REFUSALS = [
    (dict(t=32769), {}, "slots"), (dict(t=2048, top_k=2, e=8), {}, "rows per expert"),(dict(top_k=9), {}, "top_k"), (dict(dtype=torch.float32), {}, "float16 / bfloat16"), (dict(wdtype=torch.float64), {}, "weights must be"),
    (dict(h=192), {}, "multiple of 128"), (dict(e=1025), {}, "experts"), (dict(t=5), dict(tile_rows=32), "tile_rows"),
    (dict(up=_stack(4, 256, 512)), {}, "one expert count"), (dict(gate=_stack(4, 256, 384, zeros=False)), {}, "all have packed zero points"),
]


@pytest.mark.parametrize("kw,opt,word", PLAN_REFUSALS, ids=[r[2] for r in PLAN_REFUSALS])
def test_plan_gives_the_reason_it_refuses(kw, opt, word):
    with pytest.raises(ops.QllmUnsupported, match=re.escape(word)):
        ops.moe_prefill_plan(*_plan_args(**kw), **opt)


def test_the_built_kernels_use_no_scratch():
    kernels = {k: v for k, v in resources("moe_prefill.hip").items() if "moe_" in k}
    assert sum("moe_prefill_gemm_kernel" in k for k in kernels) == 8 and any("moe_route_kernel" in k for k in kernels) and any("moe_combine_kernel" in k for k in kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
