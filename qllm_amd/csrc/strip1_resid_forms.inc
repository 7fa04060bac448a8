// What strip1_resid.hip and strip1_swiglu_resid.hip share: the launch of one RESID form, the forms of one (NW, MAXS) pair, the pair table
// and the launcher.  Included once by each, with QLLM_RESID_KERNEL the family's kernel template (<NW, MAXS, EXACT, G64, B3, WAVES>,
// strip1_kernel.hpp) and QLLM_RESID_LAUNCH the name of its launcher (kernels.hpp): one text to keep in step with strip1.hip's table.
namespace qllm {

// Everything up to the launcher is local to the including translation unit: the two units instantiate the same template names around
// different kernels, and with external linkage the linker would keep ONE ResidForms<NW, MAXS>::launch for both
namespace {

// Second launch bound (minimum waves per SIMD) per form: the twin's (plain or SWIGLU: the same rule).  The residual element is ONE more live register from the load
// batch to the epilogue; every form keeps it without scratch inside its twin's bound (-Rpass-analysis=kernel-resource-usage; DESIGN 3.12
// has the table): 64 registers (8 waves per SIMD) for the plain forms up to rounds of 24 k-steps, 128 (4) for the rest.
template <int MAXS, bool G64, bool B3>
constexpr int resid_form_waves() {
  return (MAXS <= 24 && !G64 && !B3) ? 8 : 4;
}

template <int NW, int MAXS, bool EXACT, bool G64 = false, bool B3 = false>
static int launch_t(const Strip1Params &p, int n_strips, hipStream_t stream) {
  constexpr int lds_bytes = strip1_lds_bytes<NW, MAXS, 1>();
  static_assert(lds_bytes <= 160 * 1024, "LDS of one CU");
  constexpr int waves = resid_form_waves<MAXS, G64, B3>();
  if constexpr (lds_bytes > 64 * 1024) {
    static DeviceLatch attr_done;
    if (int rc = lds_optin(attr_done, (const void *)QLLM_RESID_KERNEL<NW, MAXS, EXACT, G64, B3, waves>)) return rc;
  }
  hipLaunchKernelGGL((QLLM_RESID_KERNEL<NW, MAXS, EXACT, G64, B3, waves>), dim3(n_strips, 1), dim3(NW * 64), lds_bytes, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// the batch-1 forms of one (NW, MAXS) pair, as launch_e of strip1.hip picks them
template <int NW, int MAXS>
struct ResidForms {
  static int launch(const Strip1Params &p, int n_strips, hipStream_t stream) {
    const bool exact = NW * MAXS == p.T;
    if (p.bits3) {  // 3-bit layers: 64- and 128-wide groups, rounds of up to 32 k-steps
      if constexpr (MAXS <= 32) {
        if (p.group64) return exact ? launch_t<NW, MAXS, true, true, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, true, true>(p, n_strips, stream);
        return exact ? launch_t<NW, MAXS, true, false, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, false, true>(p, n_strips, stream);
      } else {
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 3-bit layers on the batch-1 kernel stop at K = 16384");
      }
    }
    if (p.group64) {  // 64-wide groups: rounds of up to 48 k-steps
      if constexpr (MAXS <= 48)
        return exact ? launch_t<NW, MAXS, true, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, true>(p, n_strips, stream);
      else
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 64-wide groups on the batch-1 kernel stop at K = 24576");
    }
    return exact ? launch_t<NW, MAXS, true>(p, n_strips, stream) : launch_t<NW, MAXS, false>(p, n_strips, stream);
  }
};

}  // namespace

// every (NW, MAXS) pair of launch_strip1's table (strip1.hip)
#define QLLM_RESID_PAIRS(X) \
  X(4, 8) X(4, 16) X(4, 32) X(8, 16) X(7, 16) X(8, 24) X(8, 32) X(16, 16) X(16, 24) X(15, 24) X(16, 32) X(16, 40) X(16, 48) X(16, 56) X(16, 64)

int QLLM_RESID_LAUNCH(const Strip1Params &p, int nw, int maxs, int n_strips, hipStream_t stream) {
  if (p.M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "internal: the fused residual forms take one row");
#define X(NW, MAXS) \
  if (nw == NW && maxs == MAXS) return ResidForms<NW, MAXS>::launch(p, n_strips, stream);
  QLLM_RESID_PAIRS(X)
#undef X
  return set_error(QLLM_ERR_UNSUPPORTED, "fused residual: no batch-1 instantiation for nw=%d round=%d", nw, maxs);
}

}  // namespace qllm
