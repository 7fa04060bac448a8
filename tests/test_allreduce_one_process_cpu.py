"""The host side of tests/test_allreduce_one_process_gpu.py, without a GPU: the premise of its expected sums, the staging buffer's layout
against the library's own size, and the fused entry's refusal of a batch-1 shape that has no all-reduce instantiation."""
import ctypes as C

import numpy as np
import pytest

from allreduce_world import CTL_BYTES, MAX_WORLD, Layout, expected_sum, mixed_vectors, narrow, narrow_accumulator_sum, widen
from qllm_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("world", [3, 5, 8, 16])
def test_expected_sum_tells_order_and_accumulator_width_apart(world, dt):
    """The GPU tests compare with no tolerance, so they can only fail on a wrong order or a narrow accumulator if the right answer differs
    from those: on mixed_vectors it does, in at least a tenth of the elements."""
    n = 8200
    v = mixed_vectors(world, n, dt, seed=world)
    want = expected_sum(v, dt)
    reverse = expected_sum(v, dt, order=range(world - 1, -1, -1))
    narrow16 = narrow_accumulator_sum(v, dt)
    assert np.isfinite(widen(want, dt)).all()
    assert (want != reverse).mean() >= 0.1, (want != reverse).mean()
    assert (want != narrow16).mean() >= 0.1, (want != narrow16).mean()
    # every rank's vector matters: leaving one out changes the result
    for r in (0, world // 2, world - 1):
        assert (want != expected_sum(v[:r] + v[r + 1:], dt)).mean() >= 0.1, r


def test_expected_sum_rounds_once_to_nearest_even():
    one = np.array([0x3C00], dtype=np.uint16)                       # fp16 1.0; 2^-11 is half an ulp of 1.0, 2^-12 a quarter
    half_ulp, quarter = narrow(np.float32([2.0 ** -11]), "f16"), narrow(np.float32([2.0 ** -12]), "f16")
    assert expected_sum([one, half_ulp], "f16")[0] == 0x3C00          # a tie: to even
    assert expected_sum([one, half_ulp, quarter], "f16")[0] == 0x3C01   # fp32 kept the quarter: above the tie (a 16-bit accumulator: 0x3C00)
    assert narrow_accumulator_sum([one, half_ulp, quarter], "f16")[0] == 0x3C00
    b1 = np.array([0x3F80], dtype=np.uint16)                        # bf16 1.0: half an ulp is 2^-8
    assert expected_sum([b1, narrow(np.float32([2.0 ** -8]), "bf16")], "bf16")[0] == 0x3F80
    assert expected_sum([b1, narrow(np.float32([2.0 ** -8]), "bf16"), narrow(np.float32([2.0 ** -10]), "bf16")], "bf16")[0] == 0x3F81
    # a world of one is the identity on finite values that are not -0
    for dt in ("f16", "bf16"):
        v = mixed_vectors(1, 4096, dt, seed=1)
        assert np.array_equal(expected_sum(v, dt), v[0])


@pytest.mark.parametrize("world", [1, 2, 16])
def test_layout_offsets_match_the_library(lib, world):
    """csrc/kernels.hpp CommCtl behind 2 x world slots: the helper's offsets against qllm_comm_buffer_bytes"""
    assert lib.qllm_comm_buffer_bytes(1, 0) == CTL_BYTES == (2 * MAX_WORLD + 2) * 4
    for slot in (16, 16384, 65536):
        lay = Layout(world, slot)
        assert lay.total == lib.qllm_comm_buffer_bytes(world, slot)
        assert lay.slot(0, 0) == 0 and lay.slot(1, 0) == world * slot and lay.slot(1, world - 1) + slot == lay.payload == 2 * world * slot
        assert lay.flag(0, 0) == lay.payload and lay.flag(1, 0) == lay.payload + 4 * MAX_WORLD
        assert lay.flag(1, MAX_WORLD - 1) + 4 == lay.epoch and lay.epoch + 4 == lay.ticket and lay.ticket + 4 == lay.total
        offs = [lay.slot(p, r) for p in (0, 1) for r in range(world)]
        assert offs == sorted(offs) and all(b - a == slot for a, b in zip(offs, offs[1:]))      # disjoint, dense, in (parity, rank) order
        assert lay.region(lay.slot(1, world - 1) + 5) == f"slot[1][{world - 1}] byte 5" and lay.region(lay.flag(1, 3)) == "flag[1][3]"
        assert lay.region(lay.epoch) == "epoch" and lay.region(lay.ticket) == "ticket" and "guard" in lay.region(-1) and "guard" in lay.region(lay.total)


@pytest.mark.parametrize("layout", [_lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z])
def test_fused_allreduce_refuses_k_18944(lib, layout):
    """A native 4-bit g128 layer with K = 18944 passes the entry's gate -- the planner puts it on the batch-1 kernel (16 waves x 40) -- but
    no all-reduce instantiation exists for that form: UNSUPPORTED, and nothing is launched (fake, aligned pointers suffice)."""
    w = _lib.QllmWeight(16, 16, 16, None, None, 18944, 4096, 128, 4, layout, 0)
    buf = C.create_string_buffer(256)
    assert lib.qllm_plan_describe(C.byref(w), 1, 1, 1, buf, 256) == 0, _lib.last_error()
    assert buf.value.decode().startswith("strip1 nw=16 round=40 "), buf.value
    rc = lib.qllm_linear_forward_allreduce(C.byref(w), 4096, 8192, 1, _lib.DT_F16, 12288, 0, 1, 1 << 20, None, None)
    assert rc == _lib.QLLM_ERR_UNSUPPORTED, (rc, _lib.last_error())
    assert "no batch-1 instantiation for nw=16 round=40" in _lib.last_error()


def test_sixteen_waves_of_sixteen_k_steps_can_be_planned(lib):
    """launch_strip1_allreduce builds 16 waves x 16 k-steps, which the shape table takes only under QLLM_S1_T256_NW16: the knob is
    settable, so the release library can reach (and the GPU tests launch) those two instantiations."""
    from qllm_amd import ops
    buf = C.create_string_buffer(256)

    def plan(K):
        w = _lib.QllmWeight(16, 16, 16, None, None, K, 8192, 128, 4, _lib.LAYOUT_NATIVE, 0)
        assert lib.qllm_plan_describe(C.byref(w), 1, 1, 1, buf, 256) == 0, _lib.last_error()
        return buf.value.decode()

    try:
        assert plan(8192).startswith("strip1 nw=8 round=32 exact ") and plan(6656).startswith("strip1 nw=8 round=32 grid")
        ops.set_knob("QLLM_S1_T256_NW16", 1)
        assert plan(8192).startswith("strip1 nw=16 round=16 exact ") and plan(6656).startswith("strip1 nw=16 round=16 grid")
        assert plan(6144).startswith("strip1 nw=8 round=24 exact ") and plan(8320).startswith("strip1 nw=16 round=24 grid")   # its neighbours stay
        with pytest.raises(Exception, match="0..1"):
            ops.set_knob("QLLM_S1_T256_NW16", 2)
    finally:
        ops.reset_knobs()
    assert plan(8192).startswith("strip1 nw=8 round=32 exact ")
