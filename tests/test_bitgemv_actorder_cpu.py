"""Act-order GPTQ layers at 2 / 5 / 6 / 7 / 8 bits without a GPU: the reference's fixtures (tests/golden/actorder_bits, minted by
tests/golden/make_goldens_actorder_bits.py) pin the oracle bit for bit; qllm_linear_forward_permuted refuses what it does not serve
before any device work (fake, aligned, never-dereferenced pointers); the gathering instantiations (csrc/bitgemv_ao.hip) use no
scratch and keep the resident blocks per CU of their bitgemv_kernel twins."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import ref_cpu as O
from conftest import load_golden
from qllm_amd import _lib

AO_FIXTURES = ["gptq_w2_g64_actorder", "gptq_w5_g64_actorder_bias", "gptq_w6_g128_actorder", "gptq_w7_g64_actorder",
               "gptq_w8_g128_actorder_sym"]


def load_ao(name):
    return load_golden("actorder_bits/" + name)


# ---- the fixtures pin the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AO_FIXTURES)
def test_fixture_pins_the_oracle_bit_for_bit(name):
    g = load_ao(name)
    assert g["layout"] == "GPTQ" and O.is_act_order(g["g_idx"], g["groupsize"])
    assert g["K"] // g["groupsize"] >= 4 and g["N"] == 128 and g["K"] in (256, 512)
    assert np.array_equal(np.bincount(g["g_idx"], minlength=g["K"] // g["groupsize"]), np.full(g["K"] // g["groupsize"], g["groupsize"]))
    qw, qz = O.pack_gptq(g["q"], g["zeros"], g["bits"], g["compat"])
    assert qw.dtype == g["qweight"].dtype and np.array_equal(qw, g["qweight"])
    assert qz.shape == g["qzeros"].shape and np.array_equal(qz, g["qzeros"])
    assert np.array_equal(O.gptq_int_weight(g["qweight"], g["bits"], g["K"]), g["q"])
    w = O.dequant("GPTQ", g["qweight"], g["scales"], g["qzeros"], g["g_idx"], g["bits"], g["groupsize"], g["K"], g["compat"])
    assert w.dtype == np.float16 and np.array_equal(w.view(np.uint16), g["W_fwd"].view(np.uint16))
    y = O.forward("GPTQ", g["x"], g["qweight"], g["scales"], g["qzeros"], g["g_idx"], g["bias"], g["bits"], g["groupsize"], g["K"],
                  g["compat"]).numpy()
    assert O.rel_err(y, g["y"]) <= 1e-3


def test_fixture_set_covers_the_widths_a_bias_and_a_symmetric_grid():
    gs = [load_ao(n) for n in AO_FIXTURES]
    assert sorted(g["bits"] for g in gs) == [2, 5, 6, 7, 8]
    assert any(g["bias"] is not None for g in gs)
    assert any((g["zeros"] == 2 ** (g["bits"] - 1)).all() for g in gs)


# ---- validation through the C ABI ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def W(bits=8, K=1024, N=256, g=128, layout=_lib.LAYOUT_GPTQ, g_idx=None):
    return _lib.QllmWeight(4096, 8192, 12288, g_idx, None, K, N, g, bits, layout, 0)


def call(lib, w, perm=16384, x=20480, y=24576, m=1):
    return lib.qllm_linear_forward_permuted(C.byref(w), perm, x, y, m, _lib.DT_F16, None, 0, None)


def test_permuted_forward_rejects_bad_arguments(lib):
    for kw in (dict(perm=None), dict(perm=16384 + 4), dict(x=None), dict(y=None)):
        assert call(lib, W(), **kw) == _lib.QLLM_ERR_INVALID, (kw, _lib.last_error())
    assert call(lib, W(g_idx=28672)) == _lib.QLLM_ERR_INVALID
    assert "g_idx" in _lib.last_error()


def test_permuted_forward_refuses_what_the_matvec_does_not_serve(lib):
    assert call(lib, W(bits=4, layout=_lib.LAYOUT_AWQ_GEMM)) == _lib.QLLM_ERR_UNSUPPORTED
    assert "qllm_gather_columns" in _lib.last_error() and "qllm_dequant" in _lib.last_error()
    assert call(lib, W(), m=17) == _lib.QLLM_ERR_UNSUPPORTED
    assert "qllm_gather_columns" in _lib.last_error()
    assert call(lib, W(K=1040)) == _lib.QLLM_ERR_UNSUPPORTED      # K % 32 != 0
    assert call(lib, W(g=48, K=960)) == _lib.QLLM_ERR_UNSUPPORTED  # group_size % 32 != 0


def test_permuted_forward_follows_the_bitgemv_knob(lib):
    try:
        assert lib.qllm_set_knob(b"QLLM_BITGEMV", 0) == 0
        assert call(lib, W()) == _lib.QLLM_ERR_UNSUPPORTED
        assert "QLLM_BITGEMV" in _lib.last_error() and "qllm_gather_columns" in _lib.last_error()
    finally:
        lib.qllm_reset_knobs()
    v, is_set = C.c_int32(0), C.c_int32(0)
    assert lib.qllm_get_knob(b"QLLM_BITGEMV", C.byref(v), C.byref(is_set)) == 0 and is_set.value == 0


# ---- resources of the gathering instantiations -------------------------------------------------------------------------------
def _blocks_per_cu(vgprs):
    """512-thread blocks resident on a CU as far as the registers decide: 512 VGPRs per lane and SIMD in granules of 8 -> waves per
    SIMD; a block is 8 waves over 4 SIMDs."""
    return (512 // ((vgprs + 7) // 8 * 8)) * 4 // 8


def test_gathering_matvec_never_spills_and_keeps_its_twins_occupancy():
    from kernel_resources import asm_text, resources
    key = lambda n: re.search(r"ILi(\d+)ELi(\d+)E", n).groups()  # noqa: E731  (BITS, MT)
    ao = {key(n): v for n, v in resources("bitgemv_ao.hip").items() if "bitgemv_ao_kernel" in n}
    plain = {key(n): v for n, v in resources("bitgemv.hip").items() if "bitgemv_kernel" in n}
    assert len(ao) == 35 and sorted(ao) == sorted(plain)
    assert not any("bitgemv_kernel" in n for n in resources("bitgemv_ao.hip"))
    text = asm_text("bitgemv_ao.hip")
    assert "scratch_" not in text
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))
    for k, r in ao.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_count"] <= 256, (k, r)
        assert _blocks_per_cu(r["vgpr_count"]) == _blocks_per_cu(plain[k]["vgpr_count"]), (k, r["vgpr_count"], plain[k]["vgpr_count"])


def test_kernel_resources_tool_lists_the_new_unit():
    import os
    from tools import kernel_asm
    mk = open(os.path.join(kernel_asm.CSRC, "Makefile")).read()
    assert "bitgemv_ao.hip" in re.search(r"^SRCS\s*:=\s*(.+)$", mk, re.M).group(1).split()
