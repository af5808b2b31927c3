/* gs_scratch.h -- what the host side of a builder or a reader holds for the length of one call: device scratch that frees
 * itself, timing events, a file staged into HBM.  Definitions that are not trivial: gs_host.hip. */
#ifndef GS_SCRATCH_H
#define GS_SCRATCH_H

#include "gs_common.h"

#include <chrono>

double gs_ms_since(std::chrono::steady_clock::time_point t0);

/* Device allocations of one call, all freed by the destructor unless handed on.  get(bytes) allocates bytes + 16: never an
 * empty allocation, and a kernel that loads whole 16-byte words may read past the last byte.  Out of memory: the sticky
 * error is cleared, "out of device memory", GS_ERR_NOMEM; anything else: GS_ERR_DEVICE. */
struct gs_scratch {
  std::vector<void *> p;
  gs_scratch() = default;
  gs_scratch(const gs_scratch &) = delete;
  gs_scratch &operator=(const gs_scratch &) = delete;
  ~gs_scratch();
  gs_status get(size_t bytes, void **out);
  template <class T>
  gs_status get(size_t bytes, T **out) {
    void *q = nullptr;
    const gs_status rc = get(bytes, &q);
    *out = (T *)q;
    return rc;
  }
  void keep(const void *q); /* the caller owns q from here on */
  template <class T>
  void drop(T *&q) { /* frees q now */
    keep(q);
    (void)hipFree(q);
    q = nullptr;
  }
};

/* rocPRIM's protocol - ask with a null temporary how much the call needs, make room, run - around ONE argument list:
 * `call` is [&](void *tmp, size_t &bytes) { return rocprim::...(tmp, bytes, ...); }, `what` names the site in messages.
 * The run with a temporary does not look at the size it is given, so no form runs before the need is known to fit. */
inline gs_status gs_prim_fail(const char *what, hipError_t e, size_t need, size_t room) {
  if (e != hipSuccess)
    gs_set_error(std::string(what) + ": " + hipGetErrorString(e));
  else
    gs_set_error(std::string(what) + ": the temporary holds " + std::to_string(room) + " bytes, the call needs " + std::to_string(need));
  return GS_ERR_DEVICE;
}
template <class F>
gs_status gs_prim_need(const char *what, F &call, size_t &need) {
  need = 0;
  const hipError_t e = call(nullptr, need);
  return e == hipSuccess ? GS_OK : gs_prim_fail(what, e, 0, 0);
}
template <class F>
gs_status gs_prim_run(const char *what, void *tmp, size_t room, size_t need, F &call) {
  if (!tmp || need > room) return gs_prim_fail(what, hipSuccess, need, room);
  const hipError_t e = call(tmp, need);
  return e == hipSuccess ? GS_OK : gs_prim_fail(what, e, 0, 0);
}
/* the temporary is carved out of a larger allocation sized up front: `room` bytes at tmp.  A need beyond it is an error */
template <class F>
gs_status gs_prim_carved(const char *what, void *tmp, size_t room, F &&call) {
  size_t need;
  GS_TRY(gs_prim_need(what, call, need));
  return gs_prim_run(what, tmp, room, need, call);
}
/* the temporary grows: a buffer of a handle or a decoder ... */
template <class F>
gs_status gs_prim(const char *what, gs_buffer &tmp, F &&call) {
  size_t need;
  GS_TRY(gs_prim_need(what, call, need));
  GS_TRY(gs_reserve(tmp, need + 16));
  return gs_prim_run(what, tmp.p, tmp.cap, need, call);
}
/* ... or an allocation in a scratch, dropped and got again when the call needs more than it holds */
struct gs_prim_tmp {
  void *p = nullptr;
  size_t bytes = 0;
};
template <class F>
gs_status gs_prim(const char *what, gs_scratch &mem, gs_prim_tmp &tmp, F &&call) {
  size_t need;
  GS_TRY(gs_prim_need(what, call, need));
  if (!tmp.p || need > tmp.bytes) {
    tmp.bytes = 0;
    if (tmp.p) mem.drop(tmp.p);
    GS_TRY(mem.get(need, &tmp.p));
    tmp.bytes = need;
  }
  return gs_prim_run(what, tmp.p, tmp.bytes, need, call);
}

/* N events; elapsed(): the milliseconds from event from[i] to event from[i] + 1, for n pairs */
gs_status gs_events_elapsed(const hipEvent_t *e, const int *from, int n, double *out);
template <int N>
struct gs_events {
  hipEvent_t e[N] = {};
  gs_events() = default;
  gs_events(const gs_events &) = delete;
  gs_events &operator=(const gs_events &) = delete;
  ~gs_events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  gs_status elapsed(const int *from, int n, double *out) const { return gs_events_elapsed(e, from, n, out); }
};

/* A file's bytes in HBM.  open() reads `path` through two page-locked chunks of `chunk` bytes - one is being read into
 * while the other's copy to the device is under way - on a non-blocking stream of its own, and returns when the last copy
 * has arrived; the chunks are released by then.  d_raw and the stream live as long as the object.  Not a regular file, or a
 * short read: "cannot read PATH", GS_ERR_IO.  ms_read: the time spent in fread; ms_wait: waiting for copies. */
struct gs_staged_file {
  void *d_raw = nullptr;
  uint64_t size = 0;
  hipStream_t st = nullptr;
  double ms_read = 0, ms_wait = 0;
  gs_scratch mem;
  ~gs_staged_file();
  gs_status open(int device, const char *path, uint64_t chunk);
};

#endif
