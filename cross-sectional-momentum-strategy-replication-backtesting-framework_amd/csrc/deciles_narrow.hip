// deciles_narrow.hip -- the per-date qcut kernel for rows of a few thousand assets (C2 / C3
// and the C5 bootstrap batches: 30k rows of 5k assets per launch).  Same algorithm and results
// as the wide-row kernel (csrc/deciles.inc); 256 threads, 1024 buckets and 1024 candidates
// use a quarter of its LDS, so four times as many rows are in flight per CU -- the per-row
// serial phases (range, targets, selection, edges) dominate at this width.
#include "csm_common.h"

#define DEC_THREADS 256
#define HB 1024
#define CAP 1024     // candidates of the target buckets (refinement splits beyond)
#define DEC_MINB 6   // 6 workgroups per CU (8: register spills, slower)
namespace dec_narrow {
#include "deciles.inc"
}  // namespace dec_narrow

bool launch_deciles_narrow(const DecLaunch& a) {
  return dec_nb_dispatch(a, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    dec_launch(a.v2 ? dec_narrow::k_deciles<NB, true, false> : dec_narrow::k_deciles<NB, false, false>,
               DEC_THREADS, a, nullptr, nullptr, nullptr);
  });
}
