// flat_model.h — what the two static executors (resnet_exec.cpp: ResNet-50, bresnet_exec.cpp: BResNet-50) share around the
// model itself: the flat parameter / gradient / buffer layout and its tensor table, the workspace arena, the backward segments
// and the gradient buckets reduced behind them, the weight-gradient side stream, and the bodies of the C-ABI entry points that
// only read or set those.  Each executor's context derives from FlatModel; nothing here depends on which one it is — what differs
// (side-stream priority, event ring size, the error-message prefix) is passed in.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "comm.h"
#include "common.h"

namespace mi355 {

struct TensorInfo {
  std::string name;
  int kind = 0;  // 0 parameter (offset into the flat params / grads), 1 buffer (offset into the flat buffers)
  size_t offset = 0;
  int ndim = 0;
  int shape[4] = {0, 0, 0, 0};  // torch logical shape, zero beyond ndim
};

// workspace planner: every slot gets its own 256-byte aligned range of ONE allocation; `slots` are resolved once it exists
struct Arena {
  size_t size = 0;
  std::vector<std::pair<void**, size_t>> slots;
  template <typename P>
  void add(P** p, size_t bytes) {
    slots.push_back({reinterpret_cast<void**>(p), size});
    size += align_up(bytes, 256);
  }
};

struct FlatModel {
  FlatModel() = default;
  FlatModel(const FlatModel&) = delete;
  FlatModel& operator=(const FlatModel&) = delete;
  ~FlatModel();  // synchronises and destroys the side stream, destroys its events, frees the arena

  // ---- layout (device < 0: layout-only context, no HIP call and no memory) ----
  int device = 0, dtype = 0, N = 0, H = 0, W = 0, num_classes = 0;
  std::vector<TensorInfo> tensors;
  size_t param_elems = 0, buffer_elems = 0;
  float *params = nullptr, *grads = nullptr, *buffers = nullptr;  // caller-owned (bind)
  char* arena = nullptr;
  size_t arena_bytes = 0;

  // ---- backward segments: [begin, end) of the flat gradient array each one completes, in backward order ----
  std::vector<std::pair<size_t, size_t>> segs;

  // ---- gradient collective inside the boundary (comm.cpp): buckets of consecutive backward segments, each reduced by one mean
  // all-reduce on the communicator's stream as soon as its last segment has been enqueued on both streams ----
  struct Bucket {
    size_t begin, end;
    int last_seg;
  };
  mi355_comm* comm = nullptr;
  std::vector<Bucket> buckets;
  bool grad_sync = true;    // false: backward skips the bucket all-reduces (DDP.no_sync(): non-final accumulation micro-steps)
  bool comm_dirty = false;  // an all-reduce of this backward call is in flight on the communicator's stream
  std::vector<Bucket> plan_buckets(size_t cap_elems) const;
  int after_segment(int seg, hipStream_t s);  // segment `seg` is enqueued on both streams: reduce the buckets it completes
  int finish(hipStream_t s);                  // end of a backward call: side stream and collective joined to `s`

  // ---- weight-gradient side stream (MI355_WGRAD_STREAM=0: overlap off, everything on the caller's stream) ----
  bool overlap = false;
  bool w_dirty = false;  // work was forked to the side stream since the last join
  hipStream_t wstream = nullptr;
  std::vector<hipEvent_t> fork_ev;  // event ring of fork / join
  size_t fork_next = 0;
  bool create_side_stream(bool highest_priority, int ring);  // false: creation failed (the destructor cleans up)
  int fork(hipStream_t s, hipStream_t* w);  // *w: the stream the next side work goes to, ordered after everything issued to `s`
  int join(hipStream_t s);                  // everything issued to the side stream becomes visible to `s`
};

// bodies of the shared C-ABI entry points; `who` ("resnet50" / "bresnet50") prefixes the error messages
int flat_num_tensors(const FlatModel* m);
int flat_tensor_info(const FlatModel* m, const char* who, int idx, char* name, int name_cap, int* kind, size_t* offset, int* ndim,
                     int* shape);
size_t flat_param_elems(const FlatModel* m);
size_t flat_buffer_elems(const FlatModel* m);
size_t flat_workspace_bytes(const FlatModel* m);
int flat_bind(FlatModel* m, const char* who, float* params, float* grads, float* buffers);
int flat_num_segments(const FlatModel* m);
int flat_segment_range(const FlatModel* m, const char* who, int seg, size_t* grad_begin, size_t* grad_end);
int flat_bucket_plan(const FlatModel* m, const char* who, double bucket_cap_mb, int cap, int* n_out, size_t* begins, size_t* ends,
                     int* last_segs);
int flat_set_comm(FlatModel* m, const char* who, mi355_comm* comm, double bucket_cap_mb);
int flat_set_grad_sync(FlatModel* m, const char* who, int on);

}  // namespace mi355
