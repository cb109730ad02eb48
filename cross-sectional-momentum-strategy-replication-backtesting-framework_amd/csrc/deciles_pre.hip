// deciles_pre.hip -- the per-date qcut kernel of the fused pipeline (csm_deciles_ids /
// csm_pipeline): the wide-row kernel of csrc/deciles.inc in PRE mode, reading the fixed-map
// bucket ids csm_signal_ids wrote (M is read only for the few cells near a bin edge).  Its own
// translation unit so the kernel builds in parallel with the other sources.
#include "csm_common.h"

// (overridable for same-box A/B builds: -DDEC_PRE_THREADS=256 -DDEC_PRE_HB=4096 ...)
#ifndef DEC_PRE_THREADS
#define DEC_PRE_THREADS 512
#endif
#ifndef DEC_PRE_HB
#define DEC_PRE_HB 8192
#endif
#ifndef DEC_PRE_CAP
#define DEC_PRE_CAP 4096
#endif
#define DEC_THREADS DEC_PRE_THREADS
#define HB DEC_PRE_HB
#define CAP DEC_PRE_CAP
#define DEC_LU 8
#define DEC_CHUNK_ORDER 1   // merged pass summed in the split pass's order (deciles.inc)
namespace dec_pre {
#include "deciles.inc"
}  // namespace dec_pre

bool launch_deciles_pre(const DecLaunch& a, int64_t cells) {
  // merged pass first (flg): one sweep of ids + next_ret per row (deciles.inc, MG); then the
  // general kernel takes the rows it left (all rows without flg) -- and, LS given, its last
  // workgroup forms the long-short (deciles_wide.hip launches k_long_short instead for these rows).
  // (The merged pass with the general path as an in-workgroup fallback needs more than the 128
  // VGPRs of two 512-thread workgroups per CU at this width.)
  // (the merged pass sums in the split pass's order: its chunks of `cells` cells)
  return dec_nb_dispatch(a, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (a.flg) {
      DecSplit sp{};
      sp.cells = cells;
      dec_launch(dec_pre::k_deciles<NB, true, true, true>, DEC_THREADS, a, a.flg, nullptr, nullptr, sp);
    }
    dec_launch(dec_pre::k_deciles<NB, true, true, false>, DEC_THREADS, a, a.flg, a.LS, a.ticket);
  });
}

// the split pass: plan -> chunked sweep -> finish (+ the general kernel for the rows the plan or
// a sweep chunk left, FLG = 1) -- deciles.inc's split section
bool launch_deciles_split(const DecLaunch& a, const DecSplit& sp) {
  return dec_nb_dispatch(a, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    dec_launch(dec_pre::k_deciles<NB, true, true, true, false, 1>, DEC_THREADS, a, a.flg, nullptr,
               nullptr, sp);
    hipLaunchKernelGGL((sp.pf ? dec_pre::k_dsplit_sweep<NB, true> : dec_pre::k_dsplit_sweep<NB, false>),
                       dim3((unsigned)sp.C, (unsigned)a.T_m), dim3(SPLIT_THREADS), 0, a.st, a.NR,
                       (const uint16_t*)a.ids, a.N, a.L, a.flg, sp);
    // the finish launch: the listed cells of the rows the plan and sweep took, the general path
    // for the rows they left; LS given, its last workgroup forms the long-short
    dec_launch(dec_pre::k_deciles<NB, true, true, false, false, 2>, DEC_THREADS, a, a.flg, a.LS,
               a.ticket, sp);
  });
}
