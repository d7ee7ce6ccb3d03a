// qsim_core.h -- error plumbing, the chunk handle and its argument checks.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
// ------------------------------------------------------------------ error plumbing
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(e_ == hipErrorOutOfMemory ? QSIM_ERR_NOMEM : QSIM_ERR_HIP,          \
                  "%s failed: %s", #expr, hipGetErrorString(e_));                     \
  } while (0)

// ------------------------------------------------------------------ chunk handle
struct qsim_chunk {
  int device;
  int k;                 // log2(amplitudes)
  double2* amp;          // device pointer
  hipStream_t stream;
  bool owns_memory;
  qsim_chunk* parent;    // for views (keeps nothing alive; caller orders destruction)
  hipEvent_t ev0, ev1;   // timing
  bool have_events;
  double* scratch;       // reduction partials and the dense block's matrix: 64 KiB (lazily allocated, owned)
  void* work;            // the readout workspace: what the last readout call laid out in it (ensure_work: grown on demand, owned)
  u64 work_bytes;
  int last_passes;       // HBM passes of the last qsim_apply_ops
  u64 span_bytes;        // size of the allocation the chunk lives in (cache-policy choice)
  struct SplitIo* split;         // split form of qsim_apply_ops_io: what is planned but not yet launched (abi_pending.h; owned)
  bool own_in_chunk;     // the last qsim_apply_ops_io stored its own slab into THIS chunk (dst_own == src, one pass): qsim_apply_ops_io_own_slab
  struct DeferredTail* deferred;  // the tail of a cyclic plan that has not run yet (abi_pending.h settle; owned)
};

static const int kMaxDevices = 16;
static hipStream_t g_stream[kMaxDevices];
static bool g_stream_ready[kMaxDevices];
static std::mutex g_mu;

static int device_stream(int device, hipStream_t* out) {
  std::lock_guard<std::mutex> lock(g_mu);
  if (device < 0 || device >= kMaxDevices) return fail(QSIM_ERR_INVALID, "device %d out of range", device);
  if (!g_stream_ready[device]) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&g_stream[device], hipStreamNonBlocking));
    g_stream_ready[device] = true;
  }
  *out = g_stream[device];
  return QSIM_OK;
}

static inline u64 amps(const qsim_chunk* c) { return 1ull << c->k; }

// `nt` (run time) -> the kernels' NT template argument: the statement once for each value.
#define QSIM_WITH_NT(...)                               \
  do {                                                  \
    if (nt) { constexpr bool NT = true; __VA_ARGS__; }  \
    else { constexpr bool NT = false; __VA_ARGS__; }    \
  } while (0)

// ------------------------------------------------------------------ argument checks
// Every exported call that takes a chunk comes through check_chunk before it touches or hands out the amplitudes, so this
// is where the deferred tail of a cyclic plan runs (abi_pending.h settle): nobody sees a state with the tail missing.
// Calls that overwrite the whole state drop the tail instead (check_chunk_overwritten), qsim_apply_cycle looks at it itself.
static int settle(qsim_chunk* c);
static int check_chunk_unsettled(const qsim_chunk* c, const char* what) {
  if (!c || !c->amp) return fail(QSIM_ERR_INVALID, "%s: null chunk", what);
  return QSIM_OK;
}
static int check_chunk(const qsim_chunk* c, const char* what) {
  const int rc = check_chunk_unsettled(c, what);
  return rc ? rc : settle(const_cast<qsim_chunk*>(c));
}

static int check_local_qubit(const qsim_chunk* c, int q) {
  if (q < 0) return fail(QSIM_ERR_INVALID, "qubit %d is negative", q);
  if (q >= c->k)
    return fail(QSIM_ERR_NONLOCAL,
                "qubit %d >= log2(chunk_size)=%d: non-local gate requires layout/collect step",
                q, c->k);
  return QSIM_OK;
}

static int check_group(qsim_chunk* const* cs, int n, const char* what) {
  for (int i = 0; i < n; ++i) {
    int rc = check_chunk(cs[i], what);
    if (rc) return rc;
    if (cs[i]->k != cs[0]->k) return fail(QSIM_ERR_INVALID, "%s: chunks differ in size", what);
    if (cs[i]->device != cs[0]->device)
      return fail(QSIM_ERR_INVALID, "%s: chunks live on different devices", what);
    for (int j = 0; j < i; ++j)
      if (cs[i]->amp == cs[j]->amp) return fail(QSIM_ERR_INVALID, "%s: the same chunk twice", what);
  }
  return QSIM_OK;
}
