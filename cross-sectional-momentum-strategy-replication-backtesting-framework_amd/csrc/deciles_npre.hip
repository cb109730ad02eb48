// deciles_npre.hip -- the sweeps' decile pass on bucket ids (csm_momentum_multi_ids ->
// csm_deciles_ids on rows of <= dec_narrow_max assets): the narrow-row kernel of
// csrc/deciles.inc in PRE mode with 2048 buckets (the fixed map's ids >> 2).  Finer than the
// streaming narrow kernel's 1024 so that fewer cells share an edge's bucket: each of those costs
// a scattered 8-B read of mom_J (a cache line of HBM traffic).  Own translation unit: builds in
// parallel with the others.
#include "csm_common.h"

#define DEC_THREADS 256
#define HB 2048
#define CAP 512
#define DEC_MINB 4   // the general kernel and the merged pass with decile sums: no spills
#define DEC_MINB_MG0 8   // labels-only merged pass: 59 VGPRs, 20 KB LDS -> 8 workgroups per CU
namespace dec_npre {
#include "deciles.inc"
}  // namespace dec_npre

// the fused sweep path on bucket ids (csm_momentum_multi_ids -> csm_deciles_ids on rows of
// <= dec_narrow_max assets): merged pass, then the general PRE kernel for the rows it leaves
bool launch_deciles_pre_narrow(const DecLaunch& a) {
  // with decile sums (C2): ONE launch -- a row the merged pass gives up takes the general path
  // in the same workgroup, and LS (with the context's ticket) is formed by the last workgroup.
  // Labels only (the sweeps, NB = 0): the merged kernel keeps its 8 workgroups per CU only
  // without the general path beside it (64 VGPRs; with it the kernel spills), so the general
  // kernel follows as its own launch for the rows the merged pass left (flg[t] = 1).
  return dec_nb_dispatch(a, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if constexpr (NB > 0) {
      if (a.flg) {
        dec_launch(dec_npre::k_deciles<NB, true, true, true, true>, DEC_THREADS, a, nullptr, a.LS,
                   a.ticket);
        return;
      }
    }
    if (a.flg)
      dec_launch(dec_npre::k_deciles<NB, true, true, true>, DEC_THREADS, a, a.flg, nullptr, nullptr);
    dec_launch(dec_npre::k_deciles<NB, true, true, false>, DEC_THREADS, a, a.flg, a.LS, a.ticket);
  });
}
