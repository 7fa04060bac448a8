"""-m gpu: the routed experts above four tokens (csrc/moe_prefill.hip) through ops.moe_route / moe_prefill_gate_up / moe_prefill_down and
QuantExperts' opt-in route.  Shapes, layers, the float64 models and the derived bound are test_moe_decode_gpu's.  T = 5, 17, 70 tokens, both
tile heights forced through tile_rows; ids: distinct random experts per token, every token on the SAME top_k experts (a segment crosses tile
edges and ends ragged, other experts are empty), and the random ones with the sentinel E in some slots."""
import pytest
import torch

from test_moe_decode_cpu import tiny_checkpoint
from test_moe_decode_gpu import DEV, DTYPES, SHAPES, _bound_and_ref, _down_model, _experts, _logits_close

pytestmark = pytest.mark.gpu
CASES = [pytest.mark.parametrize("shape", SHAPES, ids=str), pytest.mark.parametrize("t", [5, 17, 70]), pytest.mark.parametrize("tile", [16, 64]),
         pytest.mark.parametrize("pattern", ["random", "same", "sentinel"])]


def cases(fn):
    for mark in CASES:
        fn = mark(fn)
    return fn


def _ids(e, top_k, t, pattern):
    g = torch.Generator().manual_seed(1000 * t + e)
    if pattern == "same":
        return torch.arange(top_k - 1, -1, -1).repeat(t, 1)          # descending: the combine must reorder
    ids = torch.stack([torch.randperm(e, generator=g)[:top_k] for _ in range(t)])
    if pattern == "sentinel":
        ids[torch.rand(t, top_k, generator=g) < 0.25] = e
    return ids.contiguous()


def _route(ids, e, hid, inter, tile):
    from qllm_amd import ops
    ws = torch.empty(ops.moe_prefill_workspace_bytes(ids.shape[0], ids.shape[1], e, hid, inter), dtype=torch.uint8, device=DEV)
    return ops.moe_route(ids, e, tile_rows=tile, workspace=ws)


@cases
def test_route_is_the_stable_sort_padded_to_tiles(shape, t, tile, pattern):
    (e, top_k, hid, inter), ids = shape, _ids(shape[0], shape[1], t, pattern)
    tiles, counts, srt, tile_expert, tile_row0 = _route(ids.to(DEV), e, hid, inter, tile).table()
    flat = ids.view(-1)
    order = torch.sort(flat, stable=True).indices
    order = order[flat[order] < e]                                   # sentinel slots are absent
    want_counts = torch.bincount(flat[flat < e], minlength=e)
    want_tiles = (want_counts + tile - 1) // tile
    want_rows, at = [], 0
    for ex in range(e):
        c = int(want_counts[ex])
        want_rows += [order[at:at + c], torch.full((int(want_tiles[ex]) * tile - c,), -1)]   # padding rows are marked
        at += c
    assert torch.equal(counts.long(), want_counts) and tiles == int(want_tiles.sum())
    assert torch.equal(srt.long(), torch.cat(want_rows))
    assert torch.equal(tile_expert.long(), torch.repeat_interleave(torch.arange(e), want_tiles))
    assert torch.equal(tile_row0.long(), torch.arange(tiles) * tile)


@pytest.mark.parametrize("w32", [True, False], ids=["w_f32", "w_act"])
@cases
@DTYPES
def test_exact_inputs_give_the_contract_bit_for_bit(dtype, shape, t, tile, pattern, w32):
    """Every fp32 sum is exact, so each kernel has ONE right answer: a wrong expert, row, tile edge or add order changes bits."""
    from qllm_amd import ops
    (e, top_k, hid, inter), (mod, w64, _) = shape, _experts(shape, True)
    gate, up, down, _ = mod._stacks
    g = torch.Generator().manual_seed(7 * t + top_k)
    ids = _ids(e, top_k, t, pattern)
    x = torch.randint(-2, 3, (t, hid), generator=g).to(dtype)
    hin = torch.randint(-2, 3, (t * top_k, inter), generator=g).to(dtype)
    wts = torch.rand(t, top_k, generator=g).to(torch.float32 if w32 else dtype)
    idd = ids.to(DEV)
    route = _route(idd, e, hid, inter, tile)
    got = ops.moe_prefill_gate_up(x.to(DEV), idd, route, gate, up).cpu()
    y = ops.moe_prefill_down(hin.to(DEV), idd, wts.to(DEV), route, down).cpu()
    flat = ids.view(-1)
    for ex in range(e):
        slots = (flat == ex).nonzero().view(-1)
        if len(slots):
            xs = x[slots // top_k].double()
            gh, uh = (xs @ w64[0][ex]).to(dtype), (xs @ w64[1][ex]).to(dtype)
            want = (torch.nn.functional.silu(gh.to(DEV)).cpu().double() * uh.double()).to(dtype)
            assert torch.equal(got[slots], want), (ex, (got[slots] != want).nonzero()[:4])
    want_y = _down_model(hin, ids, wts, w64[2], e, dtype).to(dtype)
    assert torch.equal(y, want_y), (y != want_y).nonzero()[:4]


@cases
@DTYPES
def test_realistic_values_within_the_derived_bound_on_both_routes(dtype, shape, t, tile, pattern):
    from qllm_amd import ops
    (e, top_k, hid, inter), (mod, w64, smax) = shape, _experts(shape, False)
    gate, up, down, _ = mod._stacks
    g = torch.Generator().manual_seed(11 * t + top_k)
    ids = _ids(e, top_k, t, pattern)
    x = torch.randn(t, hid, generator=g).to(dtype)
    wts = torch.softmax(torch.randn(t, top_k, generator=g), -1)
    ref, bound = _bound_and_ref(x, ids, wts, w64, smax, e, dtype)
    xd, idd, wd = x.to(DEV), ids.to(DEV), wts.to(DEV)
    route = _route(idd, e, hid, inter, tile)
    fused = ops.moe_prefill_down(ops.moe_prefill_gate_up(xd, idd, route, gate, up), idd, wd, route, down)
    loop = mod.forward_loop(xd, idd, wd)
    r_fused, r_loop = (((o.cpu().double() - ref).abs() / bound).max().item() for o in (fused, loop))
    print(f"moe_prefill {dtype} {shape} T={t} tile={tile} {pattern}: max |err| / bound fused {r_fused:.4f} loop {r_loop:.4f}")
    assert r_loop <= 1.0, "the bound is wrong: the unfused loop misses it"
    assert r_fused <= 1.0


@DTYPES
def test_a_captured_block_follows_the_contents_of_ids_and_weights(dtype):
    from qllm_amd import ops
    e, top_k, hid, inter = SHAPES[0]
    gate, up, down, _ = _experts(SHAPES[0], False)[0]._stacks
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, hid, generator=g).to(dtype).to(DEV)
    ws = torch.empty(ops.moe_prefill_workspace_bytes(5, top_k, e, hid, inter), dtype=torch.uint8, device=DEV)

    def eager(x, ids, wts):
        route = ops.moe_route(ids, e, workspace=ws)
        return ops.moe_prefill_down(ops.moe_prefill_gate_up(x, ids, route, gate, up), ids, wts, route, down)
    ids_a, ids_b = _ids(e, top_k, 5, "random").to(DEV), _ids(e, top_k, 5, "same").to(DEV)
    w_a, w_b = (torch.softmax(torch.randn(5, top_k, generator=g), -1).to(DEV) for _ in range(2))
    ids, wts = ids_a.clone(), w_a.clone()
    eager(x, ids, wts), torch.cuda.synchronize()       # warm-up outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eager(x, ids, wts)
    ids.copy_(ids_b), wts.copy_(w_b)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, eager(x, ids_b, w_b)) and not torch.equal(got, eager(x, ids_a, w_a))


@pytest.mark.parametrize("family", ["mixtral", "qwen3_moe"])
def test_a_prompt_takes_three_op_calls_per_block_and_decode_stays_the_pair(family, tmp_path, monkeypatch):
    from qllm_amd import ops
    from qllm_amd.modeling.base import load_quantized
    tiny_checkpoint(str(tmp_path), family)
    plain, model = load_quantized(str(tmp_path), device=DEV), load_quantized(str(tmp_path), device=DEV, fuse_moe_prefill=True)
    prompt, nxt = torch.tensor([[5, 9, 33, 2, 17, 40]], device=DEV), torch.tensor([[7]], device=DEV)
    calls = dict(prefill=0, decode=0, linear=0)
    for key, names in (("prefill", ("moe_route", "moe_prefill_gate_up", "moe_prefill_down")), ("decode", ("moe_gate_up", "moe_down")),
                       ("linear", ("linear_forward", "linear_forward_grouped"))):
        for name in names:
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _real=real, _key=key, **kw: (calls.__setitem__(_key, calls[_key] + 1), _real(*a, **kw))[1])
    with torch.no_grad():
        out = model(prompt, use_cache=True)
        assert calls == dict(prefill=2 * 3, decode=0, linear=0)     # two blocks, three op calls each, no matvec of the library
        model(nxt, past_key_values=out.past_key_values, use_cache=True)
        assert calls == dict(prefill=6, decode=2 * 2, linear=0)     # the following one-token step: the two decode launches
        calls.update(prefill=0, decode=0, linear=0)
        _logits_close(out.logits, plain(prompt).logits, family)
        assert calls["prefill"] == 0 and calls["linear"] > 0         # without the option: the loop
        calls.update(linear=0)
        monkeypatch.setenv("QLLM_FUSE_MOE_PREFILL", "0")
        _logits_close(out.logits, model(prompt).logits, family + " QLLM_FUSE_MOE_PREFILL=0")
        assert calls["prefill"] == 0 and calls["linear"] > 0
