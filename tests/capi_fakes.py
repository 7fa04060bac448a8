"""Fake device pointers for driving the C ABI without a GPU: aligned, distinct, never dereferenced -- every call made with them is
either refused before any device work or pure host code (the describe and workspace-size entries).  Shared by the *_cpu.py tests of the
entries with a check of their own, by tests/test_entry_contract_cpu.py and by tools/record_entry_contract.py."""
import ctypes as C

from qllm_amd import _lib

QWEIGHT, SCALES, QZEROS, X, Y = 4096, 8192, 12288, 20480, 24576
Y_STRIDE = 4096           # outputs of a group: Y, Y + Y_STRIDE, ...
PERM, NORM_WEIGHT, RSTD = 1 << 20, 2 << 20, 3 << 20
BUFLEN = 768


def W(bits=8, K=4096, N=4096, g=128, layout=_lib.LAYOUT_GPTQ, g_idx=None, qzeros=QZEROS, qweight=QWEIGHT, azb=0, scales=SCALES, bias=None):
    return _lib.QllmWeight(qweight, scales, qzeros, g_idx, bias, K, N, g, bits, layout, azb)


def arr(ws):
    return (_lib.QllmWeight * len(ws))(*ws)


def describe(lib, entry, w, m, have_ws=1):
    """The text of qllm_<entry>_describe (bitpanel, bitgemm: one descriptor; bitgroup: a list of them); the call itself must succeed."""
    buf = C.create_string_buffer(512)
    fn = getattr(lib, f"qllm_{entry}_describe")
    rc = fn(arr(w), len(w), m, have_ws, buf, 512) if entry == "bitgroup" else fn(C.byref(w), m, have_ws, buf, 512)
    assert rc == 0, _lib.last_error()
    return buf.value.decode()


# ---- one recorded call: entry name + a dict of plain arguments -> what it answered ------------------------------------------------------
# args: "w" a list of descriptor field dicts (the arguments of W; None: a NULL pointer; single-layer entries take w[0]), "n" the layer
# count passed (default len(w)), "ys" / "y", "x", "m", "dt", "have_ws", "buf" (False: NULL) and "buflen", and per entry "perm", "gate",
# "up", "act", "norm_weight", "eps", "rstd", and for the two gather entries (which take no descriptor) "k" and "perm".  Forward entries get
# no workspace and the null stream.
FORWARD_ENTRIES = ("qllm_linear_forward", "qllm_linear_forward_grouped", "qllm_linear_forward_permuted", "qllm_linear_forward_bitpanel",
                   "qllm_linear_forward_bitgemm", "qllm_linear_forward_bitgroup", "qllm_linear_forward_swiglu", "qllm_linear_forward_rmsnorm",
                   "qllm_gather_columns")
SIZE_ENTRIES = ("qllm_bitpanel_workspace_bytes", "qllm_bitgemm_workspace_bytes", "qllm_bitgroup_workspace_bytes")


def call_entry(lib, entry, args):
    """-> {"bytes": n} for a size entry, else {"rc": status, "error": qllm_last_error() of a failed call, "text": the buffer of a
    describe call that succeeded}."""
    a = dict(args)
    ws = a.get("w")
    layers = None if ws is None else [W(**f) for f in ws]
    n = a.get("n", 0 if layers is None else len(layers))
    one = None if not layers else C.byref(layers[0])
    many = None if not layers else arr(layers)
    x, y, m, dt = a.get("x", X), a.get("y", Y), a.get("m", 1), a.get("dt", _lib.DT_F16)
    ys = a.get("ys", [Y + Y_STRIDE * i for i in range(max(n, 1))])
    ys = None if ys is None else (C.c_void_p * len(ys))(*ys)
    buflen = a.get("buflen", BUFLEN)
    buf = C.create_string_buffer(BUFLEN) if a.get("buf", True) else None
    have_ws = a.get("have_ws", 1)
    fn = getattr(lib, entry)
    if entry in SIZE_ENTRIES:
        return {"bytes": fn(many, n, m) if entry == "qllm_bitgroup_workspace_bytes" else fn(one, m)}
    if entry in ("qllm_linear_forward", "qllm_linear_forward_bitpanel", "qllm_linear_forward_bitgemm"):
        rc = fn(one, x, y, m, dt, None, 0, None)
    elif entry in ("qllm_linear_forward_grouped", "qllm_linear_forward_bitgroup"):
        rc = fn(many, ys, n, x, m, dt, None, 0, None)
    elif entry == "qllm_linear_forward_permuted":
        rc = fn(one, a.get("perm", PERM), x, y, m, dt, None, 0, None)
    elif entry == "qllm_linear_forward_swiglu":
        rc = fn(one, a.get("gate", X), a.get("up", X + (1 << 16)), y, m, dt, a.get("act", _lib.ACT_SILU), None)
    elif entry == "qllm_linear_forward_rmsnorm":
        rc = fn(many, ys, n, x, a.get("norm_weight", NORM_WEIGHT), a.get("eps", 1e-5), m, dt, a.get("rstd", None), None)
    elif entry in ("qllm_bitpanel_describe", "qllm_bitgemm_describe"):
        rc = fn(one, m, have_ws, buf, buflen)
    elif entry in ("qllm_bitgroup_describe", "qllm_plan_describe"):
        rc = fn(many, n, m, have_ws, buf, buflen)
    elif entry == "qllm_swiglu_describe":
        rc = fn(one, m, buf, buflen)
    elif entry == "qllm_rmsnorm_describe":
        rc = fn(many, n, m, buf, buflen)
    elif entry == "qllm_gather_describe":
        rc = fn(m, a.get("k", 4096), buf, buflen)
    elif entry == "qllm_gather_columns":
        rc = fn(x, a.get("perm", PERM), y, m, a.get("k", 4096), dt, None)
    else:
        raise KeyError(entry)
    out = {"rc": rc}
    if rc != 0:
        out["error"] = _lib.last_error()
    elif entry not in FORWARD_ENTRIES:
        out["text"] = buf.value.decode()
    return out


def call_with_knobs(lib, entry, args, knobs=None):
    """call_entry under the knob overrides `knobs` ({name: value}), which are reset whatever happens."""
    try:
        for name, value in (knobs or {}).items():
            assert lib.qllm_set_knob(name.encode(), value) == 0, _lib.last_error()
        return call_entry(lib, entry, args)
    finally:
        if knobs:
            lib.qllm_reset_knobs()
