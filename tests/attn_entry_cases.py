"""Fake argument sets for the four attention entries of the C ABI (qllm_attn_decode / _window, qllm_attn_prefill / _window): aligned,
distinct, never-dereferenced integer "pointers" and named strides, shared by tests/test_attn_decode_cpu.py, tests/test_attn_prefill_cpu.py
and tests/test_attn_entry_rules_cpu.py -- and, for the last one, the table of faults whose answers tests/golden/attn_entry_rules.json
records: every fault alone and every pair that one argument set can carry, so that the file pins which rule wins and the whole text.

A call made with these must be refused before any device work.  decode_call leaves the workspace out unless told otherwise, so a
decode call that passes every other rule still ends at the workspace rule; prefill needs no workspace, so every prefill call made from
here carries at least one fault that no other argument can cancel (`FAULTS`: two faults of one `group`, or that set one argument, are
never paired)."""
import ctypes as C
import itertools

from qllm_amd import _lib

DECODE_PTRS = {n: 4096 * (i + 1) for i, n in enumerate(("q", "k_new", "v_new", "k_cache", "v_cache", "mask", "out", "len_dev", "ws"))}
DECODE_STRIDE_NAMES = ("q_row", "q_head", "kn_row", "kn_head", "vn_row", "vn_head", "c_batch", "c_head", "c_pos")
DECODE_STRIDES = (512, 64, 128, 64, 128, 64, 2 * 100 * 64, 100 * 64, 64)        # 8 query heads, 2 kv heads of 64, 100 positions
PREFILL_PTRS = {n: 4096 * (i + 1) for i, n in enumerate(("q", "k_cache", "v_cache", "mask", "out", "len_dev"))}
PREFILL_STRIDE_NAMES = ("q_batch", "q_head", "q_row", "c_batch", "c_head", "c_pos")
PREFILL_STRIDES = (5 * 512, 64, 512, 2 * 100 * 64, 100 * 64, 64)                # 5 rows of 8 query heads


def _strides(names, strides, kw):
    return [kw.pop(n, s) for n, s in zip(names, strides)]


def decode_call(lib, b=2, hq=8, hk=2, d=64, kv_len=10, max_len=100, strides=DECODE_STRIDES, mask_kind=_lib.ATTN_MASK_BOOL, mask_len=100, mask_batch=100,
                dt=_lib.DT_F16, ws_bytes=1 << 30, window=None, **kw):
    """qllm_attn_decode (window None) or qllm_attn_decode_window with an append and a bool mask; `kw`: pointers by name (None: NULL;
    `len_dev` and `ws` are NULL unless given) and single strides by name."""
    strides = _strides(DECODE_STRIDE_NAMES, strides, kw)
    p = dict(dict(DECODE_PTRS, len_dev=None, ws=None), **kw)
    assert set(p) == set(DECODE_PTRS), sorted(kw)
    head = (p["q"], p["k_new"], p["v_new"], p["k_cache"], p["v_cache"], p["mask"], p["out"], b, hq, hk, d, kv_len, p["len_dev"], max_len)
    tail = (*strides, mask_kind, mask_len, mask_batch, 0.125, dt, p["ws"], ws_bytes, None)
    return lib.qllm_attn_decode(*head, *tail) if window is None else lib.qllm_attn_decode_window(*head, window, *tail)


def prefill_call(lib, b=2, hq=8, hk=2, d=64, s=5, kv_len=10, max_len=100, strides=PREFILL_STRIDES, mask_kind=_lib.ATTN_MASK_BOOL, mask_len=100,
                 mask_batch=500, mask_row=100, causal=1, dt=_lib.DT_F16, window=None, **kw):
    """qllm_attn_prefill (window None) or qllm_attn_prefill_window with a bool mask; `kw` as for decode_call (`len_dev` NULL unless given)."""
    strides = _strides(PREFILL_STRIDE_NAMES, strides, kw)
    p = dict(dict(PREFILL_PTRS, len_dev=None), **kw)
    assert set(p) == set(PREFILL_PTRS), sorted(kw)
    head = (p["q"], p["k_cache"], p["v_cache"], p["mask"], p["out"], b, hq, hk, d, s, kv_len, p["len_dev"], max_len)
    tail = (*strides, mask_kind, mask_len, mask_batch, mask_row, causal, 0.125, dt, None)
    return lib.qllm_attn_prefill(*head, *tail) if window is None else lib.qllm_attn_prefill_window(*head, window, *tail)


# ---- the recorded table ------------------------------------------------------------------------------------------------------------------------
# The valid argument sets the faults are applied to: batch 2, 4 query heads, 2 kv heads, head_dim 64, 100 positions (3 rows at prefill).
BASE = {
    "decode": dict(b=2, hq=4, hk=2, d=64, kv_len=10, max_len=100, strides=(256, 64, 128, 64, 128, 64, 12800, 6400, 64)),
    "prefill": dict(b=2, hq=4, hk=2, d=64, s=3, kv_len=10, max_len=100, strides=(3 * 256, 64, 256, 12800, 6400, 64), mask_batch=300),
}
CALLS = {"decode": decode_call, "prefill": prefill_call}
SHAPE_ARGS = {"decode": ("b", "hq", "hk", "d", "max_len"), "prefill": ("b", "hq", "hk", "d", "s", "max_len")}


def _faults(kind):
    """{name: (overrides, group)}: every way one call can break a rule of the entry and its helpers (and decode's call without an
    append, which breaks none but is refused for its missing workspace)."""
    ptrs, names = (DECODE_PTRS, DECODE_STRIDE_NAMES) if kind == "decode" else (PREFILL_PTRS, PREFILL_STRIDE_NAMES)
    f = {}
    for n in ("q", "k_cache", "v_cache", "out"):
        f["null " + n] = ({n: None}, None)
        f["misaligned " + n] = ({n: ptrs[n] + 8}, None)
    for n in SHAPE_ARGS[kind]:
        f[n + " 0"] = ({n: 0}, None)
    f["kv heads that do not divide"] = (dict(hk=3), None)
    f["window -1"] = (dict(window=-1), None)
    f["act_dtype 7"] = (dict(dt=7), None)
    f["mask_kind 3"] = (dict(mask_kind=3), None)
    f["a kind without a mask"] = (dict(mask=None), "mask and kind")
    f["a mask without a kind"] = (dict(mask_kind=_lib.ATTN_MASK_NONE), "mask and kind")
    f["misaligned len_dev"] = (dict(len_dev=ptrs["len_dev"] + 4), None)
    f["misaligned additive mask"] = (dict(mask=ptrs["mask"] + 1, mask_kind=_lib.ATTN_MASK_ADDITIVE), None)
    for n in names:
        f[n + " stride 4"] = ({n: 4}, None)
        f[n + " stride -8"] = ({n: -8}, None)
    f["kv_len above max_len"] = (dict(kv_len=101), None)
    f["short mask"] = (dict(mask_len=9), None)
    f["short mask with the length on the device"] = (dict(len_dev=ptrs["len_dev"], mask_len=99), None)
    f["negative mask batch stride"] = (dict(mask_batch=-100), None)
    f["head_dim 96"] = (dict(d=96), None)
    f["group of 9"] = (dict(hq=18, hk=2), None)
    f["batch 70000"] = (dict(b=70000), None)
    if kind == "decode":
        f["k_new alone"] = (dict(v_new=None), "append pair")
        f["v_new alone"] = (dict(k_new=None), "append pair")
        # no fault: the call without an append, which ends at the workspace rule.  Alone and paired it reaches what the base never does
        # -- five strides looked at instead of nine, kv_len itself in 0..max_len, a mask that covers kv_len
        f["no append"] = (dict(k_new=None, v_new=None), "append pair")
        f["no append, kv_len above max_len"] = (dict(k_new=None, v_new=None, kv_len=101), "append pair")
        f["no append, kv_len at max_len"] = (dict(k_new=None, v_new=None, kv_len=100), "append pair")
        f["no append, the mask covers kv_len alone"] = (dict(k_new=None, v_new=None, mask_len=10), "append pair")
        f["misaligned k_new"] = (dict(k_new=ptrs["k_new"] + 8), None)
        f["misaligned v_new"] = (dict(v_new=ptrs["v_new"] + 8), None)
        f["kv_len -1"] = (dict(kv_len=-1), None)
        f["kv_len + 1 above max_len"] = (dict(kv_len=100), None)
        f["batch * kv_heads 6000"] = (dict(b=3000, hq=2, hk=2), None)
        f["no workspace"] = (dict(ws=None), None)
        f["short workspace"] = (dict(ws=ptrs["ws"], ws_bytes=16384), None)        # the counter page alone: the partial results do not fit
        f["misaligned workspace"] = (dict(ws=ptrs["ws"] + 8), None)
    else:
        f["q_len 1"] = (dict(s=1), None)
        f["q_len above max_len"] = (dict(s=101), None)
        f["kv_len below q_len"] = (dict(kv_len=2), None)
        f["negative mask row stride"] = (dict(mask_row=-1), None)
        f["causal 2"] = (dict(causal=2), None)
        f["window 3 without causal"] = (dict(window=3, causal=0), None)
        f["q_heads 70000"] = (dict(hq=70000, hk=8750), None)
    return f


FAULTS = {kind: _faults(kind) for kind in ("decode", "prefill")}


def fault_sets(kind):
    """[(id, overrides)]: every fault alone, then every unordered pair whose faults set different arguments and are not of one group."""
    f = FAULTS[kind]
    out = [(name, over) for name, (over, _) in f.items()]
    for (a, (oa, ga)), (b, (ob, gb)) in itertools.combinations(f.items(), 2):
        if not set(oa) & set(ob) and (ga is None or ga != gb):
            out.append((a + " + " + b, dict(oa, **ob)))
    return out


# six served shapes for the describe and workspace entries: (batch, q_heads, kv_heads, head_dim, q_len at prefill, max_len)
SERVED_SHAPES = ((2, 4, 2, 64, 3, 100), (1, 32, 8, 128, 300, 4096), (1, 8, 2, 64, 16, 128), (64, 32, 32, 128, 2, 4096), (3, 28, 4, 128, 129, 1027),
                 (1, 1, 1, 128, 1000, 1 << 20))


def entry_answers(lib):
    """{id: answer} of every C call of the table: [status, qllm_last_error()] of the window entries -- and the entries without a window
    are asked the same wherever the fault set names no window; they must answer alike -- and [status, error, text, workspace bytes] of
    the describe and workspace entries for the refused and the served shapes."""
    got = {}
    for kind in ("decode", "prefill"):
        for name, over in fault_sets(kind):
            args = dict(BASE[kind], **over)
            rc = CALLS[kind](lib, **dict(args, window=args.get("window", 0)))
            got[f"{kind}: {name}"] = [rc, _lib.last_error()]
            if "window" not in over:
                plain = [CALLS[kind](lib, **args), _lib.last_error()]
                assert plain == got[f"{kind}: {name}"], (kind, name, plain, got[f"{kind}: {name}"])
        shapes = [(name, dict(BASE[kind], **over)) for name, (over, _) in FAULTS[kind].items() if set(over) <= set(SHAPE_ARGS[kind])]
        shapes += [("served %d" % i, dict(zip(("b", "hq", "hk", "d", "s", "max_len"), shape))) for i, shape in enumerate(SERVED_SHAPES)]
        for name, args in shapes:
            shape = [args[n] for n in SHAPE_ARGS[kind]]
            buf = C.create_string_buffer(256)
            rc = getattr(lib, f"qllm_attn_{kind}_describe")(*shape, buf, 256)
            answer = [rc, _lib.last_error(), buf.value.decode()]
            if kind == "decode":
                answer += [lib.qllm_attn_decode_workspace_bytes(*shape), _lib.last_error()]
            got[f"{kind} describe: {name}"] = answer
    return got
