"""Build-time guard on the register budget of the kernels the default dispatch reaches (no GPU needed: hipcc
cross-compiles gfx950 to assembly and the resource usage is read from the code-object metadata).

Why: the decode kernels sit next to occupancy cliffs -- the 8-wave 64-column strip variant shares a CU between two
blocks only up to 128 VGPRs (130 cost 8 % on gate/up this round), 16-wave blocks cannot exceed 128 at all (anything more
spills), and a spilled register inside the prefill k-loop is a scratch load that also counts against vmcnt."""
import re

from kernel_resources import asm_text, resources


def _resources(src):
    return {n: (r["vgpr_count"], r["vgpr_spill_count"]) for n, r in resources(src).items()}


def _strip(nw, cpl, maxs, spg, xl, bits=4, ra=False, bf=False, mt=1, sm=False, dbg=False, oner=False):
    return (f"_ZN4qllm12strip_kernelILi{nw}ELi{cpl}ELi{maxs}ELi{spg}ELi{xl}ELi{bits}ELb{int(ra)}ELb{int(bf)}ELi{mt}ELb{int(sm)}ELb{int(dbg)}"
            f"ELb{int(oner)}EEEvNS_11StripParamsE")


def test_decode_strip_variants_fit_their_register_budget():
    res = _resources("strip.hip")
    # (kernel, max VGPRs): the launches of the headline bench and of the batch-16 / batch-32 decode paths
    budget = [
        (_strip(8, 4, 8, 4, 2), 128),             # q/k/v and gate/up grouped launches: two 8-wave blocks per CU
        (_strip(16, 1, 8, 4, 2), 128),            # o_proj
        (_strip(16, 1, 24, 4, 2), 128),           # down_proj (K = 11008 in one round of 24 loads)
        (_strip(16, 1, 8, 4, 1, ra=True), 128),   # M = 5..16, 16-column strips
        (_strip(16, 1, 8, 2, 1, ra=True), 128),   # ... g64 (HQQ)
        (_strip(8, 4, 8, 4, 1, ra=True), 256),    # M = 5..16, grouped 64-column strips
        (_strip(8, 4, 8, 2, 1, ra=True), 256),
        (_strip(16, 1, 8, 4, 1, bits=3, ra=True), 128),
        (_strip(8, 1, 8, 4, 1, ra=True, mt=2), 256),  # M = 17..32
        (_strip(8, 1, 8, 2, 1, ra=True, mt=2), 256),
    ]
    for name, cap in budget:
        assert name in res, f"kernel variant not instantiated: {name}"
        vgpr, spill = res[name]
        assert spill == 0 and vgpr <= cap, (name, vgpr, spill)


def test_no_strip_instantiation_spills():
    """Round-2 verdict: 17-133 spilled registers in instantiations outside the measured paths.  Every strip kernel that is BUILT
    (the dispatchers build only what the planner reaches) must be spill-free, in all five translation units."""
    total = 0
    for src in ("strip.hip", "strip_sm.hip", "strip_sm_ra.hip", "strip_dma_g32.hip", "strip_dma_g64.hip", "strip_dma_g128.hip"):
        res = {n: v for n, v in _resources(src).items() if "strip_kernel" in n or "strip_dma_kernel" in n}
        assert res, src
        total += len(res)
        for n, (vgpr, spill) in res.items():
            # (strip_dma.hpp counts its vmcnt queue by hand: a scratch reload there would also be one more entry on that queue)
            assert spill == 0, (src, n, vgpr, spill)
            nw = int(re.search(r"strip(?:_dma)?_kernelILi(\d+)E", n).group(1))
            assert vgpr <= (128 if nw == 16 else 256), (src, n, vgpr)   # a 16-wave block cannot exceed 128 registers
    assert total >= 100


def test_native_layout_decode_kernels_keep_their_occupancy():
    """The batch-1 strip-major kernels of the headline path, one-round forms: 8 waves x 16 k-steps at <= 64 registers (FOUR blocks
    per CU: measured 10.0-10.5 us on gate/up against 11.6-12.0 at three), the 16-wave K = 11008 form at <= 64 (two blocks)."""
    res = _resources("strip_sm.hip")
    for name, cap in ((_strip(8, 1, 16, 4, 2, sm=True, oner=True), 64), (_strip(16, 1, 24, 4, 2, sm=True, oner=True), 64),
                      (_strip(8, 1, 32, 4, 2, sm=True, oner=True), 80), (_strip(4, 1, 8, 4, 2, sm=True, oner=True), 64),
                      (_strip(8, 1, 16, 2, 2, sm=True, oner=True), 64), (_strip(8, 1, 16, 4, 2, sm=True), 80)):
        assert name in res, name
        assert res[name][1] == 0 and res[name][0] <= cap, (name, res[name])


def test_batch1_kernel_keeps_a_cu_full_of_waves():
    """csrc/strip1_kernel.hpp (round 5, the headline kernel): rounds of up to 24 k-steps at <= 64 registers (8 waves per SIMD: its
    launch bound), rounds of 32 .. 64 and the 64-wide-group forms at <= 128; the fused all-reduce forms within the same budgets; no instantiation spills."""
    res = {n: v for n, v in _resources("strip1.hip").items() if "strip1_kernel" in n}
    assert len(res) >= 16
    for n, (vgpr, spill) in res.items():
        m = re.search(r"strip1_kernelILi(\d+)ELi(\d+)E", n)
        nw, maxs = int(m.group(1)), int(m.group(2))
        # (round 6: the 64-wide-group forms carry twice the group addresses / scales, the four-row forms four sets of sums, the 3-bit forms two words per k-step: <= 128)
        tail = re.search(r"ELb([01])ELi(\d)ELb([01])EEEvNS_12Strip1ParamsE$", n)   # <..., G64, MR, B3>
        wide = tail is not None and (tail.group(1) == "1" or tail.group(2) != "1" or tail.group(3) == "1")
        assert spill == 0 and vgpr <= (64 if maxs <= 24 and not wide else 128), (n, nw, maxs, vgpr, spill)


def test_wave_specialised_prefill_kernel_budget():
    """gemm3: 4 matrix + 4 dequant waves = 2 waves per SIMD (<= 256 registers); 8 + 4 waves = 3 per SIMD (<= 168)."""
    res = _resources("gemm3.hip")
    names = [n for n in res if "gemm3_kernel" in n]
    assert len(names) == 8  # {GPTQ, AWQ} x {4 matrix waves, 4 without the priority bump, 8 matrix waves} + 3-bit rows x 8 + native bf16 (round 6)
    for n in names:
        vgpr, spill = res[n]
        cap = 256 if "ELi4ELb" in n else 168
        assert spill == 0 and vgpr <= cap, (n, vgpr, spill)


def test_prefill_kernels_do_not_spill():
    res = _resources("gemm2.hip")
    names = [n for n in res if "gemm2_kernel" in n]
    assert len(names) == 8  # {GPTQ, AWQ} x {256x128, 256x256} x {fp16, bf16 activations}
    for n in names:
        vgpr, spill = res[n]
        assert spill == 0 and vgpr <= 256, (n, vgpr, spill)


def test_panel_kernel_budget():
    """csrc/panel.hip (round 4): every instantiation that is built is spill-free; the eight-wave forms (two K halves, up to 64 rows)
    fit two waves per SIMD (<= 256 registers), the four-wave eight-row-tile forms one (<= 512).  32-wide groups stop at four row
    tiles (eight spill) and are checked to be absent above."""
    res = {n: v for n, v in _resources("panel.hip").items() if "panel_kernel" in n}
    assert len(res) >= 36  # {1, 2, 4 row tiles} x {g32, g64, g128} x {fp16, bf16} x {packed / fp16 zeros} + 8 row tiles x {g64, g128} x ...
    for n, (vgpr, spill) in res.items():
        m = re.search(r"panel_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", n)   # <row tiles, strips per wave, K halves, k-steps per group, ...>
        mt, cpl, kh, spg = (int(v) for v in m.groups())
        assert spill == 0, (n, vgpr, spill)
        assert cpl == 1 and kh == (2 if mt <= 4 else 1), n
        assert not (mt == 8 and spg == 1), n
        assert vgpr <= (256 if kh == 2 else 512), (n, vgpr)


def test_bit_stream_matvec_never_spills():
    """csrc/bitgemv.hip (round 6): 7 widths x 5 row tiles; the rounds of loads shrink with the row count so that none spills."""
    res = {n: v for n, v in _resources("bitgemv.hip").items() if "bitgemv_kernel" in n}
    assert len(res) == 35
    for n, (vgpr, spill) in res.items():
        assert spill == 0 and vgpr <= 256, (n, vgpr, spill)
    # ... and no register array may end up in scratch memory (a `break` inside an unrolled loop, or stores under per-kind branches,
    # turned the per-unit scale / zero-point arrays into private memory in the first versions: round 6)
    text = asm_text("bitgemv.hip")
    assert "scratch_load" not in text and "scratch_store" not in text
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))
