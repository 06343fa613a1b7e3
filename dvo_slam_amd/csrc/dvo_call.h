// The scaffolding of a feature entry, shared by the feature units (included at the end of dvo_internal.h): the per-device timing
// bracket behind a dvo_amd_debug_*_timing entry, the grow-and-keep device buffer, and the call's own scratch from the slab pool.
#pragma once

namespace dvo_amd {
namespace host {

// What a unit keeps per device for its dvo_amd_debug_*_timing entry (`static DeviceTiming g_timing[kMaxDevices]`): what the last
// call launched and waited for, and -- when asked for -- two events around its launches on the prep stream.
struct DeviceTiming {
  std::mutex mu;
  bool on = false;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int launches = 0, synchronisations = 0;
  double last_ms = 0.0;
  void count(int n_launches, int n_synchronisations) {
    std::lock_guard<std::mutex> lk(mu);
    launches = n_launches, synchronisations = n_synchronisations;
  }
};

// the bracket of one call: begin() before its first launch, end() behind its last, read() after the synchronisation
struct Bracket {
  DeviceTiming &t;
  bool timed;
  explicit Bracket(DeviceTiming &timing) : t(timing), timed(false) {
    std::lock_guard<std::mutex> lk(t.mu);
    timed = t.on && t.ev[0] && t.ev[1];
  }
  hipError_t begin(hipStream_t st) { return timed ? hipEventRecord(t.ev[0], st) : hipSuccess; }
  hipError_t end(hipStream_t st) { return timed ? hipEventRecord(t.ev[1], st) : hipSuccess; }
  // the bracketed device time; false: not timed, or the events cannot be read
  bool elapsed(double *ms) const {
    float f = 0.f;
    if (!timed || hipEventElapsedTime(&f, t.ev[0], t.ev[1]) != hipSuccess) return false;
    *ms = f;
    return true;
  }
  void store(double ms) {  // (a call of several brackets adds them up itself)
    std::lock_guard<std::mutex> lk(t.mu);
    t.last_ms = ms;
  }
  void read() {
    double ms;
    if (elapsed(&ms)) store(ms);
  }
  // ... and what the call launched and waited for, timed or not
  void read(int launches, int synchronisations) {
    t.count(launches, synchronisations);
    read();
  }
};

// the body of every dvo_amd_debug_*_timing entry; any of the three outputs may be NULL
inline int timing_entry(DeviceTiming *per_device, int device, int enable, int *launches, int *synchronisations, double *last_ms) {
  if (device < 0 || device >= kMaxDevices) return DVO_AMD_ERR_INVALID_ARGUMENT;
  DeviceTiming &t = per_device[device];
  if (enable) {
    const int rc = have_device();
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lk(t.mu);
  if (enable && !t.ev[0]) {
    HIP_TRY(hipSetDevice(device));
    for (hipEvent_t &e : t.ev) HIP_TRY(hipEventCreate(&e));
  }
  t.on = enable != 0;
  if (launches) *launches = t.launches;
  if (synchronisations) *synchronisations = t.synchronisations;
  if (last_ms) *last_ms = t.last_ms;
  return DVO_AMD_OK;
}

// A device buffer grown to the largest call and kept, never shrunk.  grow: at least `bytes` (and 256), rounded up to `step` (a
// power of two: 4 KiB for the graph workspaces, 64 KiB for the map and the feature tables, 1 MiB for the components area); `what`
// names the buffer in dvo_amd_last_error().  hipFree waits for whatever still reads the old buffer.
struct DeviceBuf {
  void *p = nullptr;
  size_t bytes = 0;
};

inline int grow(DeviceBuf &b, size_t bytes, size_t step, const char *what) {
  if (bytes <= b.bytes) return DVO_AMD_OK;
  if (b.p) (void)hipFree(b.p), b.p = nullptr, b.bytes = 0;
  bytes = align_up(bytes < 256 ? 256 : bytes, step);
  const hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) b.p = nullptr;
  if (e == hipErrorOutOfMemory) return DVO_AMD_ERR_OUT_OF_MEMORY;
  if (e != hipSuccess) return fail_hip(("hipMalloc (" + std::string(what) + ")").c_str(), e);
  b.bytes = bytes;
  return DVO_AMD_OK;
}

// The call's own scratch from the slab pool, given back when the Scratch goes out of scope: its owner has drained the stream by
// then, on every path.  With free_large, up to kPooledBytes are rounded up to a size the pool can hand out again (the next power
// of two from 64 KiB) and anything larger is allocated for the call and freed behind it: the pool keeps what it is given for the
// life of the process, and nothing of that size should stay parked on the device.
struct Scratch {
  static constexpr size_t kPooledBytes = (size_t)32 << 20;
  int device = 0;
  void *mem = nullptr;
  size_t bytes = 0;
  bool pooled = true;
  Scratch() = default;
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() {
    if (!mem) return;
    if (pooled)
      slab_free(device, bytes, mem);
    else
      (void)hipFree(mem);
  }
  char *base() const { return (char *)mem; }
  int take(int dev, size_t n, bool free_large = false) {
    device = dev, pooled = !free_large || n <= kPooledBytes, bytes = n;
    if (pooled) {
      if (free_large)
        for (bytes = (size_t)64 << 10; bytes < n;) bytes <<= 1;
      const int rc = slab_alloc(dev, bytes, &mem);
      if (rc) mem = nullptr;
      return rc;
    }
    if (hipMalloc(&mem, bytes) != hipSuccess) {
      (void)hipGetLastError();
      mem = nullptr;
      return DVO_AMD_ERR_OUT_OF_MEMORY;
    }
    return DVO_AMD_OK;
  }
};

}  // namespace host
}  // namespace dvo_amd
