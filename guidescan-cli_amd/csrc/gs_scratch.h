/* gs_scratch.h -- what the host side of a builder or a reader holds for the length of one call: device scratch that frees
 * itself, timing events, a file staged into HBM.  Definitions that are not trivial: gs_host.hip. */
#ifndef GS_SCRATCH_H
#define GS_SCRATCH_H

#include "gs_common.h"

#include <chrono>

#define GS_TRY(expr)                 \
  do {                               \
    gs_status rc__ = (expr);         \
    if (rc__ != GS_OK) return rc__;  \
  } while (0)

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
