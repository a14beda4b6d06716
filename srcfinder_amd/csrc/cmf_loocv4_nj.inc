// Included by cmf_loocv4_21.hip / cmf_loocv4_24.hip with SW4S_NJ defined: the k_sweep4s instantiations of one band-group count.
#include "cmf_sweep4s.h"

namespace {

// windows of 21 / 24 band groups (CO2: p = 83): the streamed kernel only -- rank 28, and rank 36 where its tables fit the LDS
// (NJ = 21: 145 KB; NJ = 24: 162 KB + the mean: does not fit, k_lowrank<24> refuses those columns).  The full-rank 4x4x4
// kernel has no room for its 13 x NJ x 64 coefficient fragments beside the W blocks beyond NJ = 18: a refused column is
// swept by the 16x16x4 kernel (sf_launch_loocv).
template <int NJ>
int launch_sweep4s_nj(const float *xt, const uint8_t *mask_t, const int32_t *nuse, const double *mu, const double *ufrag,
                      const double *wfrag2, const int32_t *lrok, const double *lam, const double *wfrag, size_t wstride,
                      const int32_t *status, const double *alphas, const SfGeom &g, int nsplit, double *part, hipStream_t st) {
  constexpr int NK1 = SF_LR_K / 4, NK2 = SF_LR_K2 / 4;
  int rows = sf_cdiv(g.lines, nsplit);
  rows = (rows + 127) / 128 * 128;
  const dim3 grid(nsplit, g.ncols);
  using S1 = SwS<NK1, NJ>;
  if (int rc = sf_lds_attr(reinterpret_cast<const void *>(k_sweep4s<NK1, 4, NJ>), S1::lds_bytes())) return rc;
  hipLaunchKernelGGL((k_sweep4s<NK1, 4, NJ>), grid, dim3(512), S1::lds_bytes(), st, xt, mask_t, nuse, mu, ufrag, wfrag2, lrok, lam,
                     wfrag, wstride, status, alphas, g.nalpha, g.lines, g.p, g.ps, rows, part, 1);
  SF_LAUNCH_CHECK("k_sweep4s");
  {
    constexpr int NK0 = SF_LR_K0 / 4;
    using S0 = SwS<NK0, NJ>;
    if (int rc = sf_lds_attr(reinterpret_cast<const void *>(k_sweep4s<NK0, 4, NJ>), S0::lds_bytes())) return rc;
    hipLaunchKernelGGL((k_sweep4s<NK0, 4, NJ>), grid, dim3(512), S0::lds_bytes(), st, xt, mask_t, nuse, mu, ufrag, wfrag2, lrok, lam,
                       wfrag, wstride, status, alphas, g.nalpha, g.lines, g.p, g.ps, rows, part, 1);
    SF_LAUNCH_CHECK("k_sweep4s(rank 24)");
  }
  // k_lowrank<NJ> (cmf_lowrank.hip) refuses the rank-36 tier for NJ = 24 and offers it for every other NJ: the two conditions are
  // ONE rule (ADVICE r5) -- a rank-36 column no launch takes would leave k_nll reading uninitialised partials
  static_assert((NJ == 24) == (SwS<NK2, NJ>::lds_bytes() > 160 * 1024),
                "rank-36 tier: the LDS fit of k_sweep4s<NK2, NJ> must agree with k_lowrank's `NJ == 24 -> refuse` (cmf_lowrank.hip)");
  if constexpr (NJ != 24) {
    using S2 = SwS<NK2, NJ>;
    if (int rc = sf_lds_attr(reinterpret_cast<const void *>(k_sweep4s<NK2, 4, NJ>), S2::lds_bytes())) return rc;
    hipLaunchKernelGGL((k_sweep4s<NK2, 4, NJ>), grid, dim3(512), S2::lds_bytes(), st, xt, mask_t, nuse, mu, ufrag, wfrag2, lrok,
                       lam, wfrag, wstride, status, alphas, g.nalpha, g.lines, g.p, g.ps, rows, part, 1);
    SF_LAUNCH_CHECK("k_sweep4s(rank 36)");
  }
  return 0;
}

}  // namespace

#define SW4S_CAT2(a, b) a##b
#define SW4S_CAT(a, b) SW4S_CAT2(a, b)
int SW4S_CAT(sf_launch_sweep4s_, SW4S_NJ)(const float *xt, const uint8_t *mask_t, const int32_t *nuse, const double *mu, const double *ufrag,
                                          const double *wfrag2, const int32_t *lrok, const double *lam, const double *wfrag, size_t wstride,
                                          const int32_t *status, const double *alphas, const SfGeom &g, int nsplit, double *part,
                                          hipStream_t st) {
  return launch_sweep4s_nj<SW4S_NJ>(xt, mask_t, nuse, mu, ufrag, wfrag2, lrok, lam, wfrag, wstride, status, alphas, g, nsplit, part, st);
}
