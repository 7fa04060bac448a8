"""No GPU: what the host side of the attention entries answers, replayed against tests/golden/attn_entry_rules.json -- the status and
the complete qllm_last_error() text of qllm_attn_decode_window / qllm_attn_prefill_window for every fault of tests/attn_entry_cases.py
alone and for every pair that one argument set can carry (so: which rule wins), the same through the entries without a window, every
describe line and workspace size for the refused and six served shapes, the complete exception text or plan tuple of
ops.attn_decode_plan / ops.attn_prefill_plan for every refusal of the two test_plan_refuses_what_the_entry_does_not_serve tests, their
pairs and a dozen served calls, and what ops.attn_decode / ops.attn_prefill raise before a launch.

The file holds results only, in the order this module generates the cases, with a digest of the case names; `record()` writes it and no
test calls it: run it on the commit whose behaviour is to be pinned (python tests/test_attn_entry_rules_cpu.py COMMIT), never on the
code under test.  The C calls are made in a child process with QLLM_NUM_CU=256 (the launch geometry depends on the compute-unit count,
which is read once per process), and only where no HIP device is visible: the pointers are fake, so a rule that stopped refusing would
launch a kernel on them."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from qllm_amd import _lib, ops

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "attn_entry_rules.json")


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def tensors(hq=4, hk=2, d=64, s=1, b=2, L=100, dtype=torch.float16):
    g = torch.Generator().manual_seed(1)
    q = torch.randn(b, s, hq, d, generator=g).to(dtype).transpose(1, 2)
    return q, torch.randn(b, hk, L, d, generator=g).to(dtype), torch.randn(b, hk, L, d, generator=g).to(dtype)


def no_inner(t):
    """`t` with its last dimension strided."""
    return t.transpose(2, 3).contiguous().transpose(2, 3)


def plan_base(kind):
    q, k, v = tensors(s=1 if kind == "decode" else 3)
    return dict(q=q, k=k, v=v, length=7, k_new=None, v_new=None, mask=None) if kind == "decode" else dict(q=q, k=k, v=v, length=7, mask=None)


def plan_refusals(kind):
    """{name: the arguments it replaces}: the refusals of test_attn_decode_cpu / test_attn_prefill_cpu's
    test_plan_refuses_what_the_entry_does_not_serve at this module's shapes."""
    s = 1 if kind == "decode" else 3
    base = plan_base(kind)
    q, k, v = base["q"], base["k"], base["v"]
    mb = torch.ones(2, 1, s, 100, dtype=torch.bool)
    qkv = lambda **kw: dict(zip("qkv", tensors(s=s, **kw)))
    kv = lambda **kw: dict(zip("kv", tensors(s=s, **kw)[1:]))
    r = {
        "fp32": dict(q=q.float(), k=k.float(), v=v.float()),
        "mixed types": dict(k=k.bfloat16()),
        "q not 4-D": dict(q=q[0]),
        "caches not 4-D": dict(k=k[0], v=v[0]),
        "caches of two shapes": dict(v=v[:, :, :99]),
        "caches of two layouts": dict(v=v.transpose(1, 2).contiguous().transpose(1, 2)),
        "another batch": dict(q=q[:1]),
        "kv heads that do not divide": kv(hk=3),
        "group of 9": dict(q=tensors(hq=18, s=s)[0]),
        "head_dim 32": qkv(d=32),
        "head_dim 96": qkv(d=96),
        "head_dim 256": qkv(d=256),
        "cache rows not contiguous": dict(k=no_inner(k), v=no_inner(v)),
        "length above the cache": dict(length=101),
        "device length int32": dict(length=torch.tensor(5, dtype=torch.int32)),
        "device length 1-D": dict(length=torch.tensor([5])),
        "short mask": dict(length=10, mask=mb[..., :9]),
        "short mask with the length on the device": dict(length=torch.tensor(5), mask=mb[..., :99]),
        "fp32 mask": dict(mask=mb.float()),
        "mask of three batch rows": dict(mask=torch.ones(3, 1, s, 100, dtype=torch.bool)),
        "mask of another row count": dict(mask=torch.ones(2, 1, s + 1, 100, dtype=torch.bool)),
        "q off 16 bytes": dict(q=torch.zeros(2 * s * 4 * 64 + 4, dtype=torch.float16)[4:].view(2, s, 4, 64).transpose(1, 2)),
    }
    if kind == "decode":
        many = lambda t: t[:1].expand(2100, *t.shape[1:])                                  # 2100 sequences x 2 kv heads: past the counter page
        r.update({
            "batch * kv_heads 4200": dict(q=many(q), k=many(k), v=many(v)),
            "k_new alone": dict(k_new=q[:, :2]),
            "two query tokens": dict(q=torch.cat((q, q), 2)),
            "length -1": dict(length=-1),
            "append at a full cache": dict(length=100, k_new=q[:, :2], v_new=q[:, 2:4]),
            "k_new of four heads": dict(k_new=q, v_new=q),
        })
    else:
        r.update({
            "one query token": dict(q=q[:, :, :1]),
            "q rows not contiguous": dict(q=no_inner(q)),
            "length below q_len": dict(length=2),
            "caches shorter than q_len": dict(k=k[:, :, :2], v=v[:, :, :2], length=2),
            "decode's 4-D mask": dict(mask=torch.ones(2, 1, 1, 100, dtype=torch.bool)),
            "decode's 2-D mask": dict(mask=torch.ones(2, 100, dtype=torch.bool)),
            "mask per head": dict(mask=torch.ones(2, 4, s, 100, dtype=torch.bool)),
            "mask rows not contiguous": dict(mask=torch.ones(2, 1, 100, s, dtype=torch.bool).transpose(2, 3)),
        })
    return r


def plan_served(kind):
    """{name: arguments}: served calls -- both q layouts, every mask form of both kinds, a 0-d int64 length, and decode's append."""
    base = plan_base(kind)
    q, k, v = base["q"], base["k"], base["v"]
    s = q.shape[2]
    mb, ma = torch.ones(2, 1, s, 100, dtype=torch.bool), torch.zeros(2, 1, s, 100, dtype=torch.float16)
    lower = (lambda m: m[:, 0, 0]) if kind == "decode" else (lambda m: m[:, 0])          # [B, L] at decode, [B, S, L] at prefill
    c = {
        "no mask": {},
        "q in the other layout": dict(q=q.transpose(1, 2)) if kind == "decode" else dict(q=q.contiguous()),
        "4-D bool mask": dict(mask=mb),
        "4-D additive mask": dict(mask=ma),
        "a view of a longer bool mask": dict(length=9, mask=mb[..., :9]),
        "bool mask without the head dimension": dict(mask=lower(mb)),
        "additive mask without the head dimension": dict(mask=lower(ma)),
        "one mask row for the batch": dict(mask=mb[:1]),
        "expanded mask": dict(mask=mb[:1].expand(2, 1, s, 100)),
        "length on the device": dict(length=torch.tensor(5)),
        "length on the device, 4-D bool mask": dict(length=torch.tensor(5), mask=mb),
        "bfloat16, one sequence, 28 / 4 heads of 128": dict(zip("qkv", tensors(hq=28, hk=4, d=128, s=s, b=1, dtype=torch.bfloat16))),
    }
    if kind == "decode":
        buf = torch.zeros(2, 1, (4 + 4) * 64, dtype=torch.float16)                         # q, k_new and v_new as slices of one row
        part = lambda lo, hi, h: buf[..., lo * 64:hi * 64].view(2, 1, h, 64).transpose(1, 2)
        c["append"] = dict(q=part(0, 4, 4), k_new=part(4, 6, 2), v_new=part(6, 8, 2), length=99)
        c["append, 4-D bool mask"] = dict(q=part(0, 4, 4), k_new=part(4, 6, 2), v_new=part(6, 8, 2), length=9, mask=mb[..., :10])
    return c


def plan_cases(kind):
    """[(id, arguments)]: each refusal, each pair of refusals that replace different arguments, then the served calls."""
    r = plan_refusals(kind)
    names = list(r)
    cases = [(n, r[n]) for n in names]
    cases += [(a + " + " + b, dict(r[a], **r[b])) for i, a in enumerate(names) for b in names[i + 1:] if not set(r[a]) & set(r[b])]
    return cases + [("served: " + n, a) for n, a in plan_served(kind).items()]


def raised(f, *a, **kw):
    try:
        got = f(*a, **kw)
    except Exception as e:   # the type is part of the record
        return [type(e).__name__, str(e)]
    return ["plan", *got]


def plan_answers():
    got = {}
    for kind, plan in (("decode", ops.attn_decode_plan), ("prefill", ops.attn_prefill_plan)):
        for name, over in plan_cases(kind):
            a = dict(plan_base(kind), **over)
            got[f"{kind}_plan: {name}"] = raised(plan, a.pop("q"), a.pop("k"), a.pop("v"), a.pop("length"), **a)
    return got


class OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: it gets an op past its device rule to the rules behind it.  Every call made with
    one must carry a fault that is refused there (here: a wrong `out`): a call that passed them would go on to load the library and
    launch on host memory.  (Built with torch.Tensor._make_subclass, which is private: if a torch release drops it, drop these cases.)"""
    is_cuda = True


def op_answers():
    """What ops.attn_decode / ops.attn_prefill raise before a launch: [exception type, text]."""
    got = {}
    for kind, op in (("decode", ops.attn_decode), ("prefill", ops.attn_prefill)):
        b = plan_base(kind)
        q, k, v = b["q"], b["k"], b["v"]
        s = q.shape[2]
        for bad in (0, -1, 2.0, "4", True):
            got[f"{kind}: window {bad!r}"] = raised(op, q, k, v, 7, window=bad)
        got[f"{kind}: CPU tensors"] = raised(op, q, k, v, 7)
        got[f"{kind}: CPU tensors, window 4"] = raised(op, q, k, v, 7, window=4)
        got[f"{kind}: a window and a refused plan"] = raised(op, q.float(), k, v, 7, window=4)
        fake = [torch.Tensor._make_subclass(OnDevice, t) for t in (q, k, v)]
        shape = (2, 4, 64) if kind == "decode" else (2, s, 4, 64)
        for name, out in (("of another shape", torch.empty(shape[::-1], dtype=q.dtype)), ("of another type", torch.empty(shape)),
                          ("not contiguous", torch.empty(shape + (2,), dtype=q.dtype)[..., 0])):
            got[f"{kind}: out {name}"] = raised(op, *fake, 7, out=out)
        if kind == "prefill":
            got["prefill: window without causal"] = raised(op, q, k, v, 7, causal=False, window=4)
            got["prefill: window 0 without causal"] = raised(op, q, k, v, 7, causal=False, window=0)
    return got


_CHILD = "import json, attn_entry_cases as c; from qllm_amd import _lib; print(json.dumps(c.entry_answers(_lib.load())))"


def entry_answers():
    env = dict(os.environ, QLLM_NUM_CU="256", PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + sys.path))
    got = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr
    return json.loads(got.stdout.strip().splitlines()[-1])


SECTIONS = {"entries": entry_answers, "plans": plan_answers, "ops": op_answers}


# ---- the file: answers in case order, every text once ------------------------------------------------------------------------------------------
def digest(ids):
    return hashlib.sha1("\n".join(ids).encode()).hexdigest()


def unpack(section, texts):
    return [[texts[x[0]] if isinstance(x, list) else x for x in answer] for answer in section["answers"]]


def record(commit):
    """Write the golden file from the build that is loaded.  Not called by any test."""
    texts, out = {}, {"recorded_at": commit, "sections": {}}
    for name, answers in SECTIONS.items():
        got = answers()
        assert name != "entries" or all(a[0] != _lib.QLLM_OK for i, a in got.items() if "describe" not in i), "a call with a fault was not refused"
        out["sections"][name] = {"cases": len(got), "digest": digest(got), "answers": [[[texts.setdefault(x, len(texts))] if isinstance(x, str) else x for x in a] for a in got.values()]}
    out["texts"] = list(texts)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    return out


def compare(name):
    golden = json.load(open(GOLDEN))
    got = SECTIONS[name]()
    section = golden["sections"][name]
    assert (len(got), digest(got)) == (section["cases"], section["digest"]), "the cases are not the recorded ones: record again on the pinned commit"
    bad = [(i, g, w) for (i, g), w in zip(got.items(), unpack(section, golden["texts"])) if g != w]
    assert not bad, f"{len(bad)} of {len(got)} answers differ from {golden['recorded_at']}, the first: {bad[0][0]!r} gave {bad[0][1]!r}, recorded {bad[0][2]!r}"
    return got


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_the_faults_and_their_pairs():
    import attn_entry_cases as c
    for kind, least in (("decode", 60), ("prefill", 48)):
        sets = c.fault_sets(kind)
        assert len(c.FAULTS[kind]) >= least and len(sets) > len(c.FAULTS[kind]) * (len(c.FAULTS[kind]) - 1) // 2 * 0.8, (kind, len(c.FAULTS[kind]), len(sets))
        assert len({name for name, _ in sets}) == len(sets)
        # no pair undoes itself: two faults on one argument, or the two halves of one rule, are never combined
        assert not any("a kind without a mask + a mask without a kind" in name or "k_new alone + v_new alone" in name for name, _ in sets)
    for kind in ("decode", "prefill"):
        assert len(plan_refusals(kind)) >= 27 and len(plan_served(kind)) >= 12 and len(plan_cases(kind)) > 200
    assert json.load(open(GOLDEN))["recorded_at"]


def test_the_plans_answer_as_recorded():
    got = compare("plans")
    assert sum(1 for a in got.values() if a[0] == "QllmUnsupported") > 400 and sum(1 for i, a in got.items() if "served: " in i and a[0] == "plan") >= 24


def test_the_ops_refuse_as_recorded():
    got = compare("ops")
    assert {a[0] for a in got.values()} == {"QllmUnsupported", "RuntimeError"}


def test_the_entries_answer_as_recorded():
    if not _lib.is_built():
        pytest.skip("library not built")
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: the entries are not called with fake pointers")
    got = compare("entries")
    served = [a for i, a in got.items() if "describe: served" in i]
    assert len(served) == 12 and all(a[0] == _lib.QLLM_OK and a[1] == "" and a[2].startswith("attn_") for a in served)


if __name__ == "__main__":
    done = record(sys.argv[1])
    print({name: s["cases"] for name, s in done["sections"].items()}, len(done["texts"]), "texts")
