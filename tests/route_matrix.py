"""One row per kernel route the planner can print: the layer(s), the call and the EXACT plan string qllm_plan_describe gives with a
workspace.  Shared by test_route_matrix_cpu.py (every row still plans the way it says, and every family / token is covered, checked
without a GPU) and test_route_memory_gpu.py (every row run under guard bands and a poisoned workspace).

`kind` is the descriptor the call streams: "GPTQ" / "HQQ" / "AWQ" -- the module's reference buffers in place -- or "NATIVE" /
"NATIVE_F16Z" -- the module's strip-major native copy (made from a GPTQ / HQQ layer).  `N` is one width, or a tuple of widths for a
sibling group sharing x (one grouped call).  Shapes are the smallest that reach the route, ragged where the route has a tail."""
from collections import namedtuple

from qllm_amd import _lib

Row = namedtuple("Row", "id kind bits g zk bias K N M dtype knobs plan act_order")

SM = " layout=strip-major"
G3 = "gemm3 tile=256x128 matrix-waves=8 staging-waves=4"

KIND_LAYOUT = {"GPTQ": _lib.LAYOUT_GPTQ, "HQQ": _lib.LAYOUT_HQQ, "AWQ": _lib.LAYOUT_AWQ_GEMM, "NATIVE": _lib.LAYOUT_NATIVE,
               "NATIVE_F16Z": _lib.LAYOUT_NATIVE_F16Z}
SOURCE_LAYOUT = {"GPTQ": "GPTQ", "HQQ": "HQQ", "AWQ": "GEMM", "NATIVE": "GPTQ", "NATIVE_F16Z": "HQQ"}   # the synthetic layer's layout


def row(id, kind, bits, g, K, N, M, plan, zk=None, bias=False, dtype="f16", knobs=None, act_order=False):
    if zk is None:
        zk = "f16" if kind in ("HQQ", "NATIVE_F16Z") else "asym"
    return Row(id, kind, bits, g, zk, bias, K, N, M, dtype, dict(knobs or {}), plan, act_order)


ROWS = [
    # ---- strip1: the batch-1 kernel (native layout), exact rounds, the four-row form, 64-wide groups at K % 128 == 64, 3 bits
    row("strip1-exact", "NATIVE", 4, 128, 4096, 1024, 1, 'strip1 nw=4 round=32 exact grid=strips x 1' + SM, bias=True),
    row("strip1-rows4", "NATIVE", 4, 128, 4096, 4096, 3, 'strip1 nw=4 round=32 exact rows=4 grid=strips x 1' + SM),
    row("strip1-g64-k4544", "NATIVE_F16Z", 4, 64, 4544, 4672, 1, 'strip1 nw=8 round=24 g64 grid=strips x 1' + SM, bias=True),
    row("strip1-bits3", "NATIVE", 3, 64, 4096, 4096, 1, 'strip1 nw=4 round=32 exact g64 bits=3 grid=strips x 1' + SM),
    # ---- strip: lds-slab (row-stream at cpl 4 / 2, native g32), register-A (row tiles 1 / 2 / 4), dma-A (cpl 1..6, row tiles 1 / 2)
    row("strip-lds-cpl4", "GPTQ", 4, 64, 4096, 11008, 1, 'strip nw=8 cpl=4 spw=16 form=lds-slab row_tiles=1', bias=True),
    row("strip-lds-cpl2-group", "GPTQ", 4, 64, 4096, (4096, 4096), 1, 'strip nw=16 cpl=2 spw=8 form=lds-slab row_tiles=1'),
    row("strip-lds-native-g32", "NATIVE", 4, 32, 4096, 4096, 1, 'strip nw=16 cpl=1 spw=8 form=lds-slab row_tiles=1' + SM),
    row("strip-ra-m5", "GPTQ", 4, 64, 4096, 11008, 5, 'strip nw=8 cpl=4 spw=16 form=register-A row_tiles=1'),
    row("strip-ra-m17", "GPTQ", 4, 128, 4096, 4096, 17, 'strip nw=8 cpl=1 spw=16 form=register-A row_tiles=2', bias=True),
    row("strip-ra-m40", "GPTQ", 4, 128, 4096, 4096, 40, 'strip nw=8 cpl=1 spw=16 form=register-A row_tiles=4'),
    row("strip-ra-native-g32", "NATIVE", 4, 32, 4096, 4096, 4, 'strip nw=16 cpl=1 spw=8 form=register-A row_tiles=1' + SM),
    row("strip-dma-bits3", "NATIVE", 3, 64, 4096, 4096, 2, 'strip nw=16 cpl=1 spw=8 form=dma-A row_tiles=1' + SM),
    row("strip-dma-cpl3", "NATIVE", 3, 64, 4096, 11008, 2, 'strip nw=8 cpl=3 spw=16 form=dma-A row_tiles=1' + SM),
    row("strip-dma-cpl2-k4544", "NATIVE", 4, 64, 4544, 4544, 3, 'strip nw=8 cpl=2 spw=18 form=dma-A row_tiles=1' + SM, bias=True),
    row("strip-dma-cpl4-group", "NATIVE_F16Z", 4, 64, 2048, (4096, 4096, 4096), 2, 'strip nw=8 cpl=4 spw=8 form=dma-A row_tiles=1' + SM),
    row("strip-dma-cpl6-group", "NATIVE", 4, 64, 4096, (11008, 11008), 2, 'strip nw=8 cpl=6 spw=16 form=dma-A row_tiles=1' + SM),
    row("strip-dma-rows2", "NATIVE", 4, 128, 4096, 4096, 17, 'strip nw=8 cpl=1 spw=16 form=dma-A row_tiles=2' + SM, bias=True),
    # ---- panel: split_k 1 / > 1, grouped, 3 bits
    row("panel-g32", "NATIVE", 4, 32, 4096, 11008, 17, 'panel cols=64 row_tiles=2 k_halves=2 split_k=1' + SM),
    row("panel-split4", "NATIVE_F16Z", 4, 128, 4096, 4096, 33, 'panel cols=64 row_tiles=4 k_halves=2 split_k=4' + SM, bias=True),
    row("panel-layers3", "NATIVE", 4, 128, 2048, (2048, 2048, 2048), 24, 'panel cols=64 row_tiles=2 k_halves=2 split_k=2 layers=3' + SM),
    row("panel-bits3-split3", "NATIVE", 3, 64, 4544, 4672, 17, 'panel cols=64 row_tiles=2 k_halves=2 split_k=3 bits=3' + SM),
    # ---- skinny: 64 / 128 column tiles, split, grouped
    row("skinny-ragged", "GPTQ", 4, 128, 1024, 1000, 1, 'skinny tile_cols=64 split_k=4 spw=2', bias=True),
    row("skinny-awq-group", "AWQ", 4, 128, 4096, (4096, 4096, 4096), 1, 'skinny tile_cols=128 split_k=6 spw=6'),
    row("skinny-g32-group", "GPTQ", 4, 32, 4096, (11008, 11008), 1, 'skinny tile_cols=64 split_k=2 spw=16'),
    # ---- bitgemv: 2 / 3 / 5 / 6 / 7 / 8 bits, split 1 / > 1
    row("bitgemv-5bit", "HQQ", 5, 64, 4096, 4096, 1, 'bitgemv bits=5 cols=32 waves=8 split_k=4', bias=True),
    row("bitgemv-8bit-m4", "GPTQ", 8, 128, 4096, 11008, 4, 'bitgemv bits=8 cols=32 waves=8 split_k=2'),
    row("bitgemv-2bit", "GPTQ", 2, 32, 3584, 18944, 1, 'bitgemv bits=2 cols=32 waves=8 split_k=1'),
    row("bitgemv-3bit", "GPTQ", 3, 32, 4096, 4096, 1, 'bitgemv bits=3 cols=32 waves=8 split_k=4'),
    row("bitgemv-6bit", "HQQ", 6, 64, 2048, 1000, 3, 'bitgemv bits=6 cols=32 waves=8 split_k=4'),
    row("bitgemv-7bit", "GPTQ", 7, 128, 2048, 1024, 1, 'bitgemv bits=7 cols=32 waves=8 split_k=4', bias=True),
    # ---- gemm: the 128x128 kernel, act-order gather
    row("gemm-ragged", "GPTQ", 4, 128, 1024, 1000, 300, 'gemm tile=128x128', bias=True),
    row("gemm-act-order", "GPTQ", 4, 128, 4096, 4096, 16, 'gemm tile=128x128 act-order-gather', act_order=True),
    # ---- gemm2: split 1 / > 1, row-stream / strip-major
    row("gemm2-g32", "GPTQ", 4, 32, 4096, 11008, 300, 'gemm2 tile=256x128 split_k=1'),
    row("gemm2-awq-split", "AWQ", 4, 128, 4096, 4096, 300, 'gemm2 tile=256x128 split_k=4', bias=True),
    row("gemm2-native", "NATIVE", 4, 32, 4096, 4096, 65, 'gemm2 tile=256x128 split_k=8' + SM),
    # ---- gemm3: plain, split_k, tail_split, the half-wide tail tile, 3 bits, grouped
    row("gemm3-awq", "AWQ", 4, 128, 4096, 4096, 2048, G3),
    row("gemm3-split", "GPTQ", 4, 32, 4096, 4096, 777, G3 + ' split_k=2', bias=True),
    row("gemm3-tail", "GPTQ", 4, 32, 4096, 11008, 777, G3 + ' tail_split=2'),
    row("gemm3-ntail-split", "NATIVE_F16Z", 4, 64, 4544, 4672, 300, G3 + ' split_k=2 n_tail=64' + SM, bias=True),
    row("gemm3-ntail-tail", "NATIVE_F16Z", 4, 64, 4544, 4672, 2048, G3 + ' tail_split=4 n_tail=64' + SM),
    row("gemm3-bits3", "GPTQ", 3, 128, 4096, 4096, 300, G3 + ' bits=3 split_k=4'),
    row("gemm3-group-tail", "GPTQ", 4, 32, 4096, (11008, 11008), 384, G3 + ' layers=2 tail_split=2'),
    row("gemm3-group-native", "NATIVE", 4, 128, 4096, (4096, 4096, 4096), 777, G3 + ' layers=3 tail_split=2' + SM, bias=True),
    # ---- bf16 activations
    row("bf16-strip1", "NATIVE", 4, 128, 4096, 1024, 1, 'strip1 nw=4 round=32 exact grid=strips x 1' + SM, dtype="bf16"),
    row("bf16-strip-dma", "NATIVE", 4, 128, 4096, 4096, 17, 'strip nw=8 cpl=1 spw=16 form=dma-A row_tiles=2' + SM, dtype="bf16"),
    row("bf16-panel", "NATIVE_F16Z", 4, 128, 4096, 4096, 33, 'panel cols=64 row_tiles=4 k_halves=2 split_k=4' + SM, dtype="bf16"),
    row("bf16-gemm3-native", "NATIVE", 4, 64, 4544, 4672, 300, G3 + ' split_k=2 n_tail=64' + SM, dtype="bf16"),
    row("bf16-gemm3-staged", "AWQ", 4, 128, 4096, 4096, 2048, G3, dtype="bf16"),
]

# Every family the planner prints, and every token that distinguishes a form: (what, regular expression on the plan, which rows).
# Each must match at least one row of that kind -- a planner change that moves a row elsewhere must move the matrix with it.
REQUIRED = [
    ("strip1 exact", r"^strip1 .* exact ", "any"),
    ("strip1 four-row form", r"^strip1 .* rows=4 ", "any"),
    ("strip1 g64 at K % 128 == 64", r"^strip1 nw=\d+ round=\d+ g64 grid", "any"),
    ("strip1 3 bits", r"^strip1 .* bits=3 ", "any"),
    ("strip1 bf16", r"^strip1 ", "bf16"),
    ("strip lds-slab, row-stream", r"^strip .*form=lds-slab row_tiles=1$", "any"),
    ("strip lds-slab, native", r"^strip .*form=lds-slab .*layout=strip-major$", "any"),
    ("strip lds-slab, grouped", r"^strip .*form=lds-slab", "group"),
    *[(f"strip register-A row_tiles={t}", rf"^strip .*form=register-A row_tiles={t}", "any") for t in (1, 2, 4)],
    ("strip register-A native", r"^strip .*form=register-A .*layout=strip-major$", "any"),
    *[(f"strip dma-A cpl={c}", rf"^strip .*cpl={c} .*form=dma-A", "any") for c in (1, 2, 3, 4, 6)],
    *[(f"strip dma-A row_tiles={t}", rf"^strip .*form=dma-A row_tiles={t}", "any") for t in (1, 2)],
    ("strip dma-A 3 bits", r"^strip .*form=dma-A", "bits3"),
    ("strip dma-A bf16", r"^strip .*form=dma-A", "bf16"),
    ("panel split_k=1", r"^panel .* split_k=1 ", "any"),
    ("panel split_k>1", r"^panel .* split_k=[2-9]", "any"),
    ("panel layers", r"^panel .* layers=\d", "group"),
    ("panel 3 bits", r"^panel .* bits=3 ", "any"),
    ("panel bf16", r"^panel ", "bf16"),
    ("skinny 64 columns", r"^skinny tile_cols=64 ", "any"),
    ("skinny 128 columns", r"^skinny tile_cols=128 ", "any"),
    ("skinny split", r"^skinny .* split_k=[2-9]", "any"),
    ("skinny grouped", r"^skinny ", "group"),
    *[(f"bitgemv {b} bits", rf"^bitgemv bits={b} ", "any") for b in (2, 3, 5, 6, 7, 8)],
    ("bitgemv split_k=1", r"^bitgemv .* split_k=1$", "any"),
    ("bitgemv split_k>1", r"^bitgemv .* split_k=[2-9]$", "any"),
    ("gemm 128x128", r"^gemm tile=128x128$", "any"),
    ("gemm act-order gather", r"^gemm tile=128x128 act-order-gather$", "any"),
    ("gemm2 split_k=1", r"^gemm2 .* split_k=1$", "any"),
    ("gemm2 split_k>1", r"^gemm2 .* split_k=[2-9]$", "any"),
    ("gemm2 strip-major", r"^gemm2 .*layout=strip-major$", "any"),
    ("gemm3 plain", r"^gemm3 tile=256x128 matrix-waves=8 staging-waves=4$", "any"),
    ("gemm3 split_k", r"^gemm3 [^b]* split_k=[2-9]$", "any"),
    ("gemm3 tail_split", r"^gemm3 .* tail_split=[2-9]$", "single"),
    ("gemm3 n_tail=64 split_k", r"^gemm3 .* split_k=[2-9] n_tail=64", "any"),
    ("gemm3 n_tail=64 tail_split", r"^gemm3 .* tail_split=[2-9] n_tail=64", "any"),
    ("gemm3 3 bits", r"^gemm3 .* bits=3", "any"),
    ("gemm3 3 bits split", r"^gemm3 .* bits=3 split_k=[2-9]", "any"),
    ("gemm3 layers + tail_split", r"^gemm3 .* layers=\d tail_split=[2-9]", "group"),
    ("gemm3 layers strip-major", r"^gemm3 .* layers=\d.*layout=strip-major$", "group"),
    ("gemm3 bf16 native (strip-major)", r"^gemm3 .*layout=strip-major$", "bf16"),
    ("gemm3 bf16, row-stream", r"^gemm3 (?!.*layout=strip-major)", "bf16"),
]


def widths(r):
    return tuple(r.N) if isinstance(r.N, tuple) else (r.N,)


def selects(r, which):
    """the rows a REQUIRED entry may be met by"""
    return {"any": True, "bf16": r.dtype == "bf16", "group": len(widths(r)) > 1, "single": len(widths(r)) == 1,
            "bits3": r.bits == 3}[which]


def act_dtype(r):
    return _lib.DT_BF16 if r.dtype == "bf16" else _lib.DT_F16


def placeholder_weights(r):
    """Descriptors for `r` with aligned fake pointers: for qllm_plan_describe / qllm_workspace_bytes_act only, never launched."""
    out = []
    for i, n in enumerate(widths(r)):
        base = 0x10000000 * (i + 1)
        zeros = None if r.zk == "sym" and r.kind in ("GPTQ", "NATIVE") else base + 0x3000
        out.append(_lib.QllmWeight(base + 0x1000, base + 0x2000, zeros, base + 0x4000 if r.act_order else None,
                                   base + 0x5000 if r.bias else None, r.K, n, r.g, r.bits, KIND_LAYOUT[r.kind], 0))
    return out
