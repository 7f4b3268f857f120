// hand_drop.hip -- the hand drop stage of the localize chains (agh_internal.h, HandDropState; DESIGN.md, "Hand filter" and "Hand
// clearance"): the one owner of the drop bytes, the lists' counters and what a chain leaves for the two counts getters.  Host code
// only: the tests themselves are hand_filter.hip and hand_clearance.hip, peers that each launch under their own setting.
#include "agh_internal.h"

#include <algorithm>

namespace agh
{
void hand_drop_release(Ctx* c)
{
  HandDropState& S = c->hand_drop;
  for (void* p : { (void*) S.d_drop, (void*) S.d_counts, (void*) S.d_views })
    if (p)
      (void) hipFree(p);
  for (void* p : { (void*) S.h_counts, (void*) S.h_views })
    if (p)
      (void) hipHostFree(p);
  S.d_drop = nullptr;
  S.d_counts = nullptr;
  S.d_views = nullptr;
  S.h_counts = nullptr;
  S.h_views = nullptr;
  S.drop_cap = 0;
}

HandDropView hand_drop_stage(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st)
{
  HandDropState& S = c->hand_drop;
  HandDropView v;
  S.filter_ran = false;
  S.clearance_ran = false;
  if (!S.filter_set && !S.clearance_set)
    return v;
  auto fail = [&v](int rc) {
    v.rc = rc;
    return v;
  };
  int rc;
  const int64_t cap = c->s_cap * 8;
  if (cap > S.drop_cap || !S.d_drop)
  {
    S.drop_cap = 0;
    if ((rc = dev_alloc(c, &S.d_drop, (size_t) std::max<int64_t>(cap, 1))))
      return fail(rc);
    S.drop_cap = std::max<int64_t>(cap, 1);
  }
  if (!S.d_counts)
  {
    void* pin = nullptr;
    if ((rc = dev_alloc(c, &S.d_counts, (size_t) kMaxClouds * kHandDropCounters)) || (rc = dev_alloc(c, &S.d_views, kHandViewTableBytes)))
      return fail(rc);
    AGH_HIPCHK_OR(c, hipHostMalloc(&pin, sizeof(int) * (size_t) kMaxClouds * kHandDropCounters, hipHostMallocDefault), fail(AGH_ERR_HIP));
    S.h_counts = static_cast<int*>(pin);
    AGH_HIPCHK_OR(c, hipHostMalloc(&pin, kHandViewTableBytes, hipHostMallocDefault), fail(AGH_ERR_HIP));
    S.h_views = static_cast<uint8_t*>(pin);
  }
  const int lists = tab ? n_lists : 1;
  for (int k = 0; k < lists * kHandDropCounters; k++)
    S.h_counts[k] = 0;
  AGH_HIPCHK_OR(c, hipMemsetAsync(S.d_counts, 0, sizeof(unsigned) * (size_t) kMaxClouds * kHandDropCounters, st), fail(AGH_ERR_HIP));
  S.filter_ran = S.filter_set;
  S.clearance_ran = S.clearance_set;
  v.drop = S.d_drop;
  v.d_counts = S.d_counts;
  v.h_counts = S.h_counts;
  if (bound <= 0)
    return v;
  // (the clearance behind a filter skips the hands it dropped; alone it writes every byte itself)
  if ((v.rc = hand_filter_launch(c, bound, tab, n_lists, st)) == AGH_OK)
    v.rc = hand_clearance_launch(c, bound, tab, n_lists, st, S.filter_ran);
  return v;
}

void hand_drop_collect(Ctx* c, int lists, const int64_t* hyp)
{
  c->hand_drop.lists = lists;
  std::copy(hyp, hyp + lists, c->hand_drop.hyp);
}

HandDropCounts hand_drop_counts(const Ctx* c, int k)
{
  // (a test that did not run left the zeros hand_drop_stage wrote)
  const int* h = c->hand_drop.h_counts + k * kHandDropCounters;
  return HandDropCounts{ c->hand_drop.hyp[k], h[kDropApproach], h[kDropWidth], h[kDropUnobserved], h[kDropClearance] };
}
}  // namespace agh
