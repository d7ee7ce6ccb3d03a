// abi_chunk.h -- C ABI: library and device queries, chunk lifetime, initial states, transfers, copies, sync, timing, launch profile.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).
extern "C" {
const char* qsim_last_error(void) { return g_err.c_str(); }
int qsim_version(void) { return 100; }

int qsim_device_count(int* count) {
  if (!count) return fail(QSIM_ERR_INVALID, "count is null");
  HIP_TRY(hipGetDeviceCount(count));
  return QSIM_OK;
}

static qsim_chunk* new_chunk(int device, int k, double2* amp, hipStream_t stream, bool owns_memory, u64 span_bytes) {
  qsim_chunk* c = new qsim_chunk();
  std::memset(c, 0, sizeof *c);
  c->device = device;
  c->k = k;
  c->amp = amp;
  c->stream = stream;
  c->owns_memory = owns_memory;
  c->span_bytes = span_bytes;
  return c;
}

int qsim_create(int device, int n_local_qubits, qsim_chunk** out) {
  if (!out) return fail(QSIM_ERR_INVALID, "out is null");
  if (n_local_qubits < 0 || n_local_qubits > 40)
    return fail(QSIM_ERR_INVALID, "n_local_qubits %d out of range [0, 40]", n_local_qubits);
  hipStream_t s;
  int rc = device_stream(device, &s);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  double2* p = nullptr;
  HIP_TRY(hipMalloc((void**)&p, sizeof(double2) << n_local_qubits));
  *out = new_chunk(device, n_local_qubits, p, s, true, sizeof(double2) << n_local_qubits);
  return QSIM_OK;
}

int qsim_create_view(qsim_chunk* parent, uint64_t offset_amps, int n_local_qubits, qsim_chunk** out) {
  int rc = check_chunk(parent, "qsim_create_view");
  if (rc) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "out is null");
  if (n_local_qubits < 0 || n_local_qubits > parent->k)
    return fail(QSIM_ERR_INVALID, "view of %d qubits does not fit a %d-qubit chunk", n_local_qubits, parent->k);
  const u64 len = 1ull << n_local_qubits;
  if (offset_amps % len != 0 || offset_amps + len > amps(parent))
    return fail(QSIM_ERR_INVALID, "view offset %llu not aligned/inside parent", (u64)offset_amps);
  *out = new_chunk(parent->device, n_local_qubits, parent->amp + offset_amps, parent->stream, false, parent->span_bytes);
  (*out)->parent = parent;
  return QSIM_OK;
}

int qsim_wrap(int device, void* device_ptr, int n_local_qubits, void* stream, qsim_chunk** out) {
  if (!out || !device_ptr) return fail(QSIM_ERR_INVALID, "null pointer");
  if (n_local_qubits < 0 || n_local_qubits > 40) return fail(QSIM_ERR_INVALID, "n_local_qubits out of range");
  if (((uintptr_t)device_ptr & 15) != 0) return fail(QSIM_ERR_INVALID, "device pointer must be 16-byte aligned");
  *out = new_chunk(device, n_local_qubits, (double2*)device_ptr, (hipStream_t)stream, false, sizeof(double2) << n_local_qubits);
  return QSIM_OK;
}

int qsim_destroy(qsim_chunk* c) {
  if (!c) return QSIM_OK;
  (void)hipSetDevice(c->device);
  if (c->have_events) { (void)hipEventDestroy(c->ev0); (void)hipEventDestroy(c->ev1); }
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->work) (void)hipFree(c->work);
  delete c->split;
  delete c->deferred;                // (a deferred tail is dropped: nobody can look at the state again)
  if (c->owns_memory && c->amp) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->amp);
  }
  delete c;
  return QSIM_OK;
}

int qsim_n_local_qubits(const qsim_chunk* c) { return c ? c->k : -1; }
// (whoever holds the pointer reads the amplitudes behind the library's back: a deferred tail runs first)
void* qsim_device_ptr(const qsim_chunk* c) { return c && settle(const_cast<qsim_chunk*>(c)) == QSIM_OK ? (void*)c->amp : nullptr; }

int qsim_init_zero(qsim_chunk* c, int set_amp0) {
  int rc = check_chunk_overwritten(c, "qsim_init_zero");
  if (rc) return rc;
  drop_pending(c);
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_fill_zero, dim3(stream_grid(amps(c))), dim3(kBlock), 0, c->stream, c->amp, amps(c), set_amp0);
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

int qsim_init_random(qsim_chunk* c, uint64_t seed) {
  int rc = check_chunk_overwritten(c, "qsim_init_random");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_fill_random, dim3(stream_grid(amps(c))), dim3(kBlock), 0, c->stream, c->amp, amps(c), (u64)seed);
  HIP_TRY(hipGetLastError());
  double n2 = 0;
  if ((rc = qsim_norm2(c, &n2))) return rc;
  if (!(n2 > 0)) return fail(QSIM_ERR_INVALID, "random state has zero norm");
  hipLaunchKernelGGL(k_scale, dim3(stream_grid(amps(c))), dim3(kBlock), 0, c->stream, c->amp, amps(c), 1.0 / std::sqrt(n2));
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

static int transfer(qsim_chunk* c, double* re_im, uint64_t offset_amps, uint64_t count, bool download) {
  // (an upload of every amplitude overwrites the state: a deferred tail is dropped, not run)
  const bool whole = !download && c && re_im && offset_amps == 0 && count == amps(c);
  int rc = whole ? check_chunk_overwritten(c, "qsim_upload") : check_chunk(c, download ? "qsim_download" : "qsim_upload");
  if (rc) return rc;
  if (!re_im && count) return fail(QSIM_ERR_INVALID, "host buffer is null");
  if (offset_amps > amps(c) || count > amps(c) - offset_amps)
    return fail(QSIM_ERR_INVALID, "%s range [%llu, +%llu) outside chunk of %llu", download ? "download" : "upload", (u64)offset_amps, (u64)count, amps(c));
  if (!count) return QSIM_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (download) HIP_TRY(hipMemcpyAsync(re_im, c->amp + offset_amps, count * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  else HIP_TRY(hipMemcpyAsync(c->amp + offset_amps, re_im, count * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QSIM_OK;
}
int qsim_upload(qsim_chunk* c, const double* re_im, uint64_t offset_amps, uint64_t count) {
  return transfer(c, const_cast<double*>(re_im), offset_amps, count, false);
}
int qsim_download(qsim_chunk* c, double* re_im, uint64_t offset_amps, uint64_t count) {
  return transfer(c, re_im, offset_amps, count, true);
}

// complex64 transfers (the reference's chunk-file dtype): converted on the device through a staging buffer
static int c64_transfer(qsim_chunk* c, float* host, uint64_t offset_amps, uint64_t count, bool download, const char* what) {
  const bool whole = !download && c && host && offset_amps == 0 && count == amps(c);
  int rc = whole ? check_chunk_overwritten(c, what) : check_chunk(c, what);
  if (rc) return rc;
  if (!host && count) return fail(QSIM_ERR_INVALID, "%s: host buffer is null", what);
  if (offset_amps > amps(c) || count > amps(c) - offset_amps)
    return fail(QSIM_ERR_INVALID, "%s: range [%llu, +%llu) outside chunk of %llu", what, (u64)offset_amps, (u64)count, amps(c));
  if (!count) return QSIM_OK;
  HIP_TRY(hipSetDevice(c->device));
  const u64 piece = std::min<u64>(count, 1ull << 24);
  float2* stage = nullptr;
  if (hipMalloc((void**)&stage, sizeof(float2) * piece) != hipSuccess) return fail(QSIM_ERR_NOMEM, "%s: no device memory for the staging buffer", what);
  hipError_t e = hipSuccess;
  for (u64 done = 0; done < count && e == hipSuccess; done += piece) {
    const u64 n = std::min<u64>(piece, count - done);
    if (download) {
      hipLaunchKernelGGL(k_to_c64, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, stage, (const double2*)(c->amp + offset_amps + done), n);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(host + 2 * done, stage, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream);
    } else {
      e = hipMemcpyAsync(stage, host + 2 * done, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(k_from_c64, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, c->amp + offset_amps + done, (const float2*)stage, n);
        e = hipGetLastError();
      }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the staging buffer is reused)
  }
  (void)hipFree(stage);
  if (e != hipSuccess) return fail(QSIM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return QSIM_OK;
}
int qsim_download_c64(qsim_chunk* c, float* re_im, uint64_t offset_amps, uint64_t count) {
  return c64_transfer(c, re_im, offset_amps, count, true, "qsim_download_c64");
}
int qsim_upload_c64(qsim_chunk* c, const float* re_im, uint64_t offset_amps, uint64_t count) {
  return c64_transfer(c, const_cast<float*>(re_im), offset_amps, count, false, "qsim_upload_c64");
}

static int launch_copy(qsim_chunk* dst, const qsim_chunk* src, bool nt) {
  constexpr int kItems = 2;
  u64 blocks = (amps(dst) + (u64)kBlock * kItems - 1) / ((u64)kBlock * kItems);
  blocks = (blocks + 7) & ~7ull;                     // whole octets: logical_block<true> deals blocks over the 8 XCDs
  QSIM_WITH_NT(hipLaunchKernelGGL((k_copy<NT, kItems>), grid_for(blocks), dim3(kBlock), 0, dst->stream, dst->amp, src->amp, amps(dst)));
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

int qsim_copy(qsim_chunk* dst, const qsim_chunk* src) {
  int rc = check_chunk(dst, "qsim_copy");
  if (rc || (rc = check_chunk(src, "qsim_copy"))) return rc;
  if (dst->k != src->k) return fail(QSIM_ERR_INVALID, "qsim_copy: sizes differ");
  if (dst->amp == src->amp) return QSIM_OK;
  HIP_TRY(hipSetDevice(dst->device));
  return launch_copy(dst, src, (sizeof(double2) << dst->k) > tuning().mall_bytes);
}

// The streaming candidates behind bench.py's `stream_ceiling`: variant 0 = qsim_copy's own choice, 1 = the non-temporal
// copy kernel whatever the size, 2 = the plain (cached) copy kernel, 3 = hipMemcpyAsync device to device (the runtime's
// blit kernel).  Measurement aid: same arguments and stream semantics as qsim_copy.
int qsim_copy_variant(qsim_chunk* dst, const qsim_chunk* src, int variant) {
  if (variant == 0) return qsim_copy(dst, src);
  int rc = check_chunk(dst, "qsim_copy_variant");
  if (rc || (rc = check_chunk(src, "qsim_copy_variant"))) return rc;
  if (dst->k != src->k) return fail(QSIM_ERR_INVALID, "qsim_copy_variant: sizes differ");
  if (dst->amp == src->amp) return fail(QSIM_ERR_INVALID, "qsim_copy_variant: source and destination are the same buffer");
  HIP_TRY(hipSetDevice(dst->device));
  if (variant == 1 || variant == 2) return launch_copy(dst, src, variant == 1);
  if (variant != 3) return fail(QSIM_ERR_INVALID, "qsim_copy_variant: variant %d", variant);
  HIP_TRY(hipMemcpyAsync(dst->amp, src->amp, sizeof(double2) << dst->k, hipMemcpyDeviceToDevice, dst->stream));
  HIP_TRY(hipGetLastError());
  return QSIM_OK;
}

// (check_chunk runs a deferred tail first: after the call the chunk holds the finished state)
int qsim_sync(qsim_chunk* c) {
  int rc = check_chunk(c, "qsim_sync");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QSIM_OK;
}

static int ensure_events(qsim_chunk* c) {
  if (!c->have_events) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    c->have_events = true;
  }
  return QSIM_OK;
}

// (the two timing calls touch no amplitude and run no deferred tail: events around executions of a cyclic plan time its
// steady passes; a region that is to pay for the tail ends in qsim_sync)
int qsim_time_begin(qsim_chunk* c) {
  int rc = check_chunk_unsettled(c, "qsim_time_begin");
  if (rc || (rc = ensure_events(c))) return rc;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  return QSIM_OK;
}

int qsim_time_end(qsim_chunk* c, float* elapsed_ms) {
  int rc = check_chunk_unsettled(c, "qsim_time_end");
  if (rc || (rc = ensure_events(c))) return rc;
  if (!elapsed_ms) return fail(QSIM_ERR_INVALID, "elapsed_ms is null");
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(elapsed_ms, c->ev0, c->ev1));
  return QSIM_OK;
}

int qsim_profile_begin(qsim_chunk* c) {
  int rc = check_chunk(c, "qsim_profile_begin");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lock(g_prof_mu);
  if (g_profs.count(c->stream)) return fail(QSIM_ERR_INVALID, "a profile is already open on this chunk's stream");
  g_profs[c->stream];
  g_prof_open.fetch_add(1);
  return QSIM_OK;
}

int qsim_profile_end(qsim_chunk* c, int max_entries, int* n_entries, qsim_profile_entry* out) {
  int rc = check_chunk(c, "qsim_profile_end");
  if (rc) return rc;
  if (!n_entries || (!out && max_entries > 0)) return fail(QSIM_ERR_INVALID, "null output");
  std::vector<LaunchRecord> records;
  {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    auto it = g_profs.find(c->stream);
    if (it == g_profs.end()) return fail(QSIM_ERR_INVALID, "no profile is open on this chunk's stream");
    records.swap(it->second.records);
    g_profs.erase(it);
    g_prof_open.fetch_sub(1);
  }
  HIP_TRY(hipSetDevice(c->device));
  hipError_t sync = hipStreamSynchronize(c->stream);
  uint64_t launches[kNumClasses] = {0}, streaming[kNumClasses] = {0};
  double ms[kNumClasses] = {0}, bytes[kNumClasses] = {0}, hbm[kNumClasses] = {0};
  hipError_t bad = sync;
  for (LaunchRecord& r : records) {
    float t = 0.f;
    if (bad == hipSuccess) bad = hipEventElapsedTime(&t, r.e0, r.e1);
    launches[r.cls] += 1;
    streaming[r.cls] += r.streaming ? 1 : 0;
    ms[r.cls] += t;
    bytes[r.cls] += r.bytes;
    hbm[r.cls] += r.hbm_bytes;
  }
  {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (LaunchRecord& r : records) { g_prof_pool.push_back(r.e0); g_prof_pool.push_back(r.e1); }
  }
  if (bad != hipSuccess) return fail(QSIM_ERR_HIP, "qsim_profile_end: %s", hipGetErrorString(bad));
  int n = 0;
  for (int cls = 0; cls < kNumClasses; ++cls) {
    if (!launches[cls]) continue;
    if (n < max_entries) {
      std::snprintf(out[n].kernel, sizeof out[n].kernel, "%s", kClassNames[cls]);
      out[n].launches = launches[cls];
      out[n].total_ms = ms[cls];
      out[n].algorithmic_bytes = bytes[cls];
      out[n].hbm_bytes = hbm[cls];
      out[n].streaming_launches = streaming[cls];
    }
    ++n;
  }
  *n_entries = n;
  return QSIM_OK;
}
}  // extern "C"
