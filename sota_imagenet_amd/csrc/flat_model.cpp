// flat_model.cpp — the plumbing both static executors share (flat_model.h).
#include "flat_model.h"

#include <algorithm>

namespace mi355 {

FlatModel::~FlatModel() {
  if (wstream) {
    (void)hipStreamSynchronize(wstream);
    (void)hipStreamDestroy(wstream);
  }
  for (hipEvent_t e : fork_ev)
    if (e) (void)hipEventDestroy(e);
  if (arena) (void)hipFree(arena);
}

// Consecutive backward segments form buckets of >= cap_elems gradient elements (summed segment sizes); a bucket is the contiguous
// span of its segments, whichever direction they run through the flat array.  The LAST bucket has nothing left to hide behind (its
// all-reduce starts when backward ends), so it is cut once more: its trailing segments up to cap_elems / 8 become a bucket of their
// own, and the part before them is reduced while those last, activation-heavy segments still compute.  parallel.plan_buckets states
// the same rule for modules without a native executor.
std::vector<FlatModel::Bucket> FlatModel::plan_buckets(size_t cap_elems) const {
  std::vector<Bucket> out;
  std::vector<int> firsts;
  const int nseg = (int)segs.size();
  auto span = [&](int f, int l) {
    size_t lo = segs[f].first, hi = segs[f].second;
    for (int i = f; i <= l; ++i) { lo = std::min(lo, segs[i].first); hi = std::max(hi, segs[i].second); }
    return Bucket{lo, hi, l};
  };
  int first = -1;
  size_t size = 0;
  for (int i = 0; i < nseg; ++i) {
    if (first < 0) { first = i; size = 0; }
    size += segs[i].second - segs[i].first;
    if (size >= cap_elems || i == nseg - 1) {
      out.push_back(span(first, i));
      firsts.push_back(first);
      first = -1;
    }
  }
  const size_t tail_cap = cap_elems / 8;
  if (!out.empty() && out.back().end - out.back().begin > tail_cap) {
    const int f = firsts.back(), l = out.back().last_seg;
    int cut = l + 1;  // first segment of the tail bucket (l + 1: no tail — the last segment alone exceeds the tail cap)
    size_t tail = 0;
    for (int i = l; i > f; --i) {
      const size_t n = segs[i].second - segs[i].first;
      if (tail + n > tail_cap) break;
      tail += n;
      cut = i;
    }
    if (cut > f && cut <= l) {
      out.back() = span(f, cut - 1);
      out.push_back(span(cut, l));
    }
  }
  return out;
}

int FlatModel::after_segment(int seg, hipStream_t s) {
  if (!comm || !grad_sync) return 0;
  for (const Bucket& bk : buckets)
    if (bk.last_seg == seg) {
      MI355_TRY(comm_allreduce_bucket(comm, grads, bk.begin, bk.end, s, overlap && w_dirty ? wstream : nullptr));
      comm_dirty = true;
    }
  return 0;
}

int FlatModel::finish(hipStream_t s) {
  MI355_TRY(join(s));
  if (comm && comm_dirty) {
    MI355_TRY(comm_join(comm, s));
    comm_dirty = false;
  }
  return 0;
}

bool FlatModel::create_side_stream(bool highest_priority, int ring) {
  bool ok;
  if (highest_priority) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    ok = hipStreamCreateWithPriority(&wstream, hipStreamNonBlocking, hi) == hipSuccess;
  } else {
    ok = hipStreamCreateWithFlags(&wstream, hipStreamNonBlocking) == hipSuccess;
  }
  fork_ev.resize(ring > 0 ? ring : 1);
  for (hipEvent_t& e : fork_ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  return ok;
}

// (a context without a side stream — overlap off, or layout-only — keeps everything on `s`: the event ring is never indexed empty)
int FlatModel::fork(hipStream_t s, hipStream_t* w) {
  if (!overlap || !wstream) {
    *w = s;
    return 0;
  }
  hipEvent_t e = fork_ev[fork_next++ % fork_ev.size()];
  MI355_HIP(hipEventRecord(e, s));
  MI355_HIP(hipStreamWaitEvent(wstream, e, 0));
  w_dirty = true;
  *w = wstream;
  return 0;
}

int FlatModel::join(hipStream_t s) {
  if (!overlap || !wstream || !w_dirty) return 0;
  hipEvent_t e = fork_ev[fork_next++ % fork_ev.size()];
  MI355_HIP(hipEventRecord(e, wstream));
  MI355_HIP(hipStreamWaitEvent(s, e, 0));
  w_dirty = false;
  return 0;
}

// ---- C-ABI bodies ---------------------------------------------------------------------------------------------------------

int flat_num_tensors(const FlatModel* m) { return m ? (int)m->tensors.size() : 0; }

int flat_tensor_info(const FlatModel* m, const char* who, int idx, char* name, int name_cap, int* kind, size_t* offset, int* ndim,
                     int* shape) {
  MI355_ARG(m && idx >= 0 && idx < (int)m->tensors.size() && name && name_cap > 0, "%s_tensor_info: bad index %d / null name", who, idx);
  const TensorInfo& t = m->tensors[idx];
  snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
  if (kind) *kind = t.kind;
  if (offset) *offset = t.offset;
  if (ndim) *ndim = t.ndim;
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  return 0;
}

size_t flat_param_elems(const FlatModel* m) { return m ? m->param_elems : 0; }
size_t flat_buffer_elems(const FlatModel* m) { return m ? m->buffer_elems : 0; }
size_t flat_workspace_bytes(const FlatModel* m) { return m ? m->arena_bytes : 0; }

int flat_bind(FlatModel* m, const char* who, float* params, float* grads, float* buffers) {
  MI355_ARG(m && params && grads && buffers, "%s_bind: null pointer", who);
  if (m->device < 0) {
    set_error("%s_bind: layout-only ctx (created with device < 0)", who);
    return MI355_E_STATE;
  }
  MI355_ARG(((uintptr_t)params % 256 == 0) && ((uintptr_t)grads % 256 == 0) && ((uintptr_t)buffers % 256 == 0),
            "%s_bind: flat arrays must be 256-byte aligned", who);
  m->params = params; m->grads = grads; m->buffers = buffers;
  return 0;
}

int flat_num_segments(const FlatModel* m) { return m ? (int)m->segs.size() : 0; }

int flat_segment_range(const FlatModel* m, const char* who, int seg, size_t* grad_begin, size_t* grad_end) {
  MI355_ARG(m && grad_begin && grad_end && seg >= 0 && seg < (int)m->segs.size(), "%s_segment_range: bad segment %d", who, seg);
  *grad_begin = m->segs[seg].first;
  *grad_end = m->segs[seg].second;
  return 0;
}

int flat_bucket_plan(const FlatModel* m, const char* who, double bucket_cap_mb, int cap, int* n_out, size_t* begins, size_t* ends,
                     int* last_segs) {
  MI355_ARG(m && n_out && bucket_cap_mb > 0, "%s_bucket_plan: bad arguments", who);
  const auto bk = m->plan_buckets((size_t)(bucket_cap_mb * (1 << 20) / 4));
  *n_out = (int)bk.size();
  for (int i = 0; i < (int)bk.size() && i < cap; ++i) {
    if (begins) begins[i] = bk[i].begin;
    if (ends) ends[i] = bk[i].end;
    if (last_segs) last_segs[i] = bk[i].last_seg;
  }
  return 0;
}

int flat_set_comm(FlatModel* m, const char* who, mi355_comm* comm, double bucket_cap_mb) {
  MI355_ARG(m && (comm == nullptr || bucket_cap_mb > 0), "%s_set_comm: bad arguments", who);
  if (m->device < 0) {
    set_error("%s_set_comm: layout-only ctx (created with device < 0)", who);
    return MI355_E_STATE;
  }
  m->comm = comm;
  m->buckets = comm ? m->plan_buckets((size_t)(bucket_cap_mb * (1 << 20) / 4)) : std::vector<FlatModel::Bucket>();
  return 0;
}

int flat_set_grad_sync(FlatModel* m, const char* who, int on) {
  MI355_ARG(m, "%s_set_grad_sync: null ctx", who);
  m->grad_sync = on != 0;
  return 0;
}

}  // namespace mi355
