// pos_rowgroup_stage.hpp -- what the runners of the grouped ingest, scrub and repair of stored files
// share on the device's side: the one twiddle table of the grouped row lengths and the
// two page-locked blocks that alternate between a call's staging groups.  The planning is
// pos_rowgroup_plan.hpp.
#pragma once
#include <functional>
#include <map>
#include <mutex>

#include "pos_internal.hpp"

namespace lcpc_host {

// the twiddles of the grouped lengths (pos_ingest_twiddles), built once per device and kept: every
// grouped entry reads this one table
inline lcpc_status pos_group_twiddles(Device *dev, hipStream_t s, const uint32_t **out) {
  static std::mutex mu;
  static std::map<int, uint32_t *> tables;
  std::lock_guard<std::mutex> lk(mu);
  auto it = tables.find(dev->id);
  if (it == tables.end()) {
    uint32_t *tw = nullptr;
    HIP_TRY(device_malloc(&tw, ((size_t)1 << POS_INGEST_MAX_LOG_ENC) * POS_WB));
    hipError_t e = pos_ingest_twiddles(tw, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(tw);
      HIP_TRY(e);
    }
    it = tables.emplace(dev->id, tw).first;
  }
  *out = it->second;
  return LCPC_OK;
}

// Two page-locked blocks for the staging groups of one call.  Group k fills block k & 1 (begin), queues
// its upload, launches and read-back into the same block, and commits what the host needs to hand the
// block's results to the jobs (Pending); that hand-over (drain) runs once the block's event has
// completed: for group k - 1 right after group k is queued, so the host works while the device does,
// and for the last group in finish().  A runner keeps this behind its device buffers, so an early
// return drains the stream before any of them is given back.
template <class Pending>
struct TwoSlotStager {
  using Drain = std::function<void(Pending &, const uint8_t *)>;
  Device *dev;
  hipStream_t s;
  Drain hand_over;  // the block's results to the jobs
  Pinned stg[2];
  Events ev;
  Pending pend[2];
  bool live[2] = {false, false};
  int k = 0;

  TwoSlotStager(Device *d, hipStream_t stream, Drain fn) : dev(d), s(stream), hand_over(std::move(fn)) {}
  // (an early return leaves copies queued on the blocks the members are about to give back)
  ~TwoSlotStager() { (void)hipStreamSynchronize(s); }

  lcpc_status drain(int slot) {
    if (!live[slot]) return LCPC_OK;
    live[slot] = false;
    HIP_TRY(hipEventSynchronize(ev.e[slot]));
    hand_over(pend[slot], stg[slot].b());
    return LCPC_OK;
  }

  // the block of the next group, `total` bytes of it, free to be written
  lcpc_status begin(size_t total, uint8_t **h) {
    const int slot = k & 1;
    HIP_TRY(ev.init());
    if (lcpc_status st = drain(slot)) return st;  // (already drained by the step before this one, but for an error there)
    if (stg[slot].n < total && !stg[slot].get(dev, total)) return fail(LCPC_ERR_OUT_OF_MEMORY, "pinned host staging");
    *h = stg[slot].b();
    return LCPC_OK;
  }

  // the group's work is queued on s: its results are p's once what is queued has completed
  lcpc_status commit(Pending &&p) {
    const int slot = k & 1;
    HIP_TRY(hipEventRecord(ev.e[slot], s));
    pend[slot] = std::move(p);
    live[slot] = true;
    k++;
    return drain(slot ^ 1);  // the group before this one, while this one runs
  }

  lcpc_status finish() {
    lcpc_status st;
    if ((st = drain(k & 1))) return st;
    if ((st = drain((k & 1) ^ 1))) return st;
    HIP_TRY(hipStreamSynchronize(s));
    return LCPC_OK;
  }
};

}  // namespace lcpc_host
