// abi_readout.h -- C ABI: what is read off a chunk without changing it: norm, outcome probabilities, Pauli-sum
// expectation values, sparse export, the closed-form checkers and the fingerprint.
// Part of the single translation unit qsim_hip.hip (included there, in order; not a standalone header).

// The r distinct local qubits of a readout call, as the mask *sel: null arguments, the range of r, pending parts, then
// qubit by qubit (range, locality, repetition).  `hint`: what follows the refusal of r (where another call serves it).
static int check_qubit_list(qsim_chunk* c, int r, const int32_t* qubits, const void* out, int min_r, int max_r, const char* what,
                            u64* sel = nullptr, const char* hint = "") {
  if (!qubits || !out) return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if (r < min_r || r > max_r) return fail(QSIM_ERR_INVALID, "%s: %d <= r <= %d qubits expected, got %d%s", what, min_r, max_r, r, hint);
  int rc = require_no_parts(c, what);
  if (rc) return rc;
  u64 mask = 0;
  if (!sel) sel = &mask;
  *sel = 0;
  for (int i = 0; i < r; ++i) {
    if ((rc = check_local_qubit(c, qubits[i]))) return rc;
    for (int j = 0; j < i; ++j) if (qubits[j] == qubits[i]) return fail(QSIM_ERR_INVALID, "%s: repeated qubit %d", what, qubits[i]);
    *sel |= 1ull << qubits[i];
  }
  return QSIM_OK;
}

// the pair checks of a call on two chunks
static int check_two_chunks(const qsim_chunk* a, const qsim_chunk* b, const char* what) {
  if (a->k != b->k) return fail(QSIM_ERR_INVALID, "%s: chunks of %d and %d index bits", what, a->k, b->k);
  if (a->device != b->device) return fail(QSIM_ERR_INVALID, "%s: chunks live on different devices", what);
  if (a->stream != b->stream) return fail(QSIM_ERR_INVALID, "%s: chunks are bound to different streams", what);
  return QSIM_OK;
}

// Do the two chunks' allocations together exceed the Infinity Cache?  (Views of one parent share its allocation.)
static bool pair_streams(const qsim_chunk* a, const qsim_chunk* b) {
  u64 bytes = a->span_bytes;
  if (a->amp != b->amp && !(a->parent && a->parent == b->parent)) bytes += b->span_bytes;
  return bytes > tuning().mall_bytes;
}

// The checks of the four Pauli-string calls, in this order: the chunks, n, null arguments, the pair (a one-chunk call
// passes its chunk twice: the pair checks then hold trivially), pending parts, then term by term locality and, where the
// call has a value per term (`value`: what it is called), that it is finite.  `noun`: "term" or "rotation".
static int check_pauli_call(const qsim_chunk* a, const qsim_chunk* b, int n, const uint64_t* x_masks, const uint64_t* z_masks,
                            const double* values, const char* value, const void* out, const int* n_passes, const char* noun,
                            const char* what) {
  int rc = check_chunk(a, what);
  if (rc || (rc = check_chunk(b, what))) return rc;
  if (n < 0) return fail(QSIM_ERR_INVALID, "%s: %s = %d", what, std::strcmp(noun, "term") ? "n" : "n_terms", n);
  if (!n_passes || (n > 0 && (!x_masks || !z_masks || !out || (value && !values))))
    return fail(QSIM_ERR_INVALID, "%s: null argument", what);
  if ((rc = check_two_chunks(a, b, what)) || (rc = require_no_parts(a, what)) || (rc = require_no_parts(b, what))) return rc;
  const u64 all = (1ull << a->k) - 1;
  for (int t = 0; t < n; ++t) {
    if ((x_masks[t] | z_masks[t]) & ~all)
      return fail(QSIM_ERR_NONLOCAL, "%s: %s %d acts on index bit %d >= log2(chunk_size)=%d", what, noun, t,
                  63 - __builtin_clzll((x_masks[t] | z_masks[t]) & ~all), a->k);
    if (value && !std::isfinite(values[t])) return fail(QSIM_ERR_INVALID, "%s: %s of %s %d is not finite", what, value, noun, t);
  }
  return QSIM_OK;
}

// qsim_plan_expectation and qsim_plan_pauli_rotations: the plan into the caller's arrays
static int plan_pauli_out(bool ordered, int k, int n, const uint64_t* x_masks, int32_t* pass_of, uint64_t* tile_masks, int* n_passes) {
  if (!n_passes || (n > 0 && (!pass_of || !tile_masks)))
    return fail(QSIM_ERR_INVALID, "%s: null argument", ordered ? "qsim_plan_pauli_rotations" : "qsim_plan_expectation");
  PauliPlan p;
  const int rc = plan_pauli(ordered, k, n, x_masks, &p);
  if (rc) return rc;
  for (int t = 0; t < n; ++t) pass_of[t] = p.pass_of[(size_t)t];
  for (size_t q = 0; q < p.tile.size(); ++q) tile_masks[q] = p.tile[q];
  *n_passes = (int)p.tile.size();
  return QSIM_OK;
}

// What qsim_expectation_pauli (width 1: a double per term) and qsim_overlap_pauli (width 2: re, im) share.  In the
// chunk's workspace: the partials | the term table | the results.  Per pass launch(q, table entries of the pass,
// partials, &rows) starts k_*_tile or k_*_wide with at most tile_wg or kExpMaxWg workgroups, and k_hist_sum adds the
// rows in workgroup order into the per-term results, in pass order; one copy to the host at the end, back in call order.
template <class Launch>
static int pauli_reduce_call(qsim_chunk* c, const PauliPasses& pp, int width, unsigned tile_wg, Launch launch, double* out, int* n_passes) {
  const u64 n = pp.slot.size(), w8 = sizeof(double) * (u64)width;
  const int np = (int)pp.plan.tile.size();
  int max_count = 1;
  for (int q = 0; q < np; ++q) max_count = std::max(max_count, pp.plan.count[(size_t)q]);
  const u64 table_off = w8 * std::max<u64>((u64)tile_wg * (u64)max_count, kExpMaxWg), out_off = table_off + ((pp.table.size() + 7) & ~7ull);
  int rc = ensure_work(c, out_off + w8 * n);
  if (rc) return rc;
  char* base = static_cast<char*>(c->work);
  double* partial = reinterpret_cast<double*>(base);
  char* dev_table = base + table_off;
  double* dev_out = reinterpret_cast<double*>(base + out_off);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(dev_table, pp.table.data(), pp.table.size(), hipMemcpyHostToDevice, c->stream));
  for (int q = 0; q < np; ++q) {
    const int first = pp.first[(size_t)q];
    unsigned rows = 0;
    if ((rc = launch(q, pp.at(dev_table, first), partial, &rows))) return rc;
    if ((rc = sum_rows(c, partial, rows, width * pp.plan.count[(size_t)q], dev_out + width * first))) return rc;
  }
  std::vector<double> res((size_t)(width * n));
  if ((rc = fetch_doubles(c, dev_out, width * n, res.data()))) return rc;
  for (u64 t = 0; t < n; ++t)
    for (int j = 0; j < width; ++j) out[width * t + j] = res[(size_t)(width * pp.slot[t] + j)];
  *n_passes = np;
  return QSIM_OK;
}

extern "C" {
int qsim_norm2(qsim_chunk* c, double* out) {
  int rc = check_chunk(c, "qsim_norm2");
  if (rc) return rc;
  if (!out) return fail(QSIM_ERR_INVALID, "out is null");
  if ((rc = ensure_scratch(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const unsigned grid = std::min<unsigned>(stream_grid(amps(c)), kReduceBlocks);
  hipLaunchKernelGGL(k_norm2_partial, dim3(grid), dim3(kBlock), 0, c->stream, c->amp, amps(c), c->scratch);
  HIP_TRY(hipGetLastError());
  return reduce_partials(c, grid, 1, false, out);
}

// Joint outcome probabilities of r measured qubits: k_hist (one read-only pass, partial histograms per workgroup) and
// k_hist_sum (the partials in workgroup order); 2^r doubles cross to the host.  Bits of the chunk index are dealt out as
// described at k_hist: 0..7 threads, then item bits, workgroup bits and loop bits, selected qubits first.
int qsim_probabilities(qsim_chunk* c, int r, const int32_t* qubits, double* out) {
  int rc = check_chunk(c, "qsim_probabilities");
  if (rc) return rc;
  u64 sel;
  if ((rc = check_qubit_list(c, r, qubits, out, 1, 8, "qsim_probabilities", &sel))) return rc;
  if ((rc = ensure_work(c, sizeof(double) * kHistDoubles))) return rc;
  double* const partial = static_cast<double*>(c->work);
  HIP_TRY(hipSetDevice(c->device));
  const int k = c->k;
  const int above = std::max(0, k - 8);
  const int n_item = std::min(3, above);
  const int n_wg = std::min(kHistWgBits, above - n_item);
  HistArgs a;
  std::memset(&a, 0, sizeof a);
  a.amp = c->amp;
  a.n = amps(c);
  a.r = r;
  for (int i = 0; i < r; ++i) a.q[i] = qubits[i];
  a.lane_sel = (int)(sel & 63);
  // selected bits above the thread bits first (item bits, then workgroup bits), then the free bits: the lowest ones as
  // item bits (a thread's loads stay close), the highest as workgroup bits (each XCD's workgroups cover one region)
  std::vector<int> hi_sel, free_bits;
  for (int b = 8; b < k; ++b) ((sel >> b) & 1 ? hi_sel : free_bits).push_back(b);
  size_t si = 0, lo = 0, hi = free_bits.size();
  u64 used = 0;
  for (int j = 0; j < n_item; ++j) { const int b = si < hi_sel.size() ? hi_sel[si++] : free_bits[lo++]; a.item_bit[j] = b; used |= 1ull << b; }
  std::vector<int> wg;
  for (int j = 0; j < n_wg; ++j) { const int b = si < hi_sel.size() ? hi_sel[si++] : free_bits[--hi]; wg.push_back(b); used |= 1ull << b; }
  if (si != hi_sel.size() || lo > hi) return fail(QSIM_ERR_INVALID, "internal: qsim_probabilities could not place the selected bits");
  std::sort(wg.begin(), wg.end());
  for (int j = 0; j < n_wg; ++j) a.wg_bit[j] = wg[(size_t)j];
  a.n_wg_bits = n_wg;
  const u64 all_hi = k > 8 ? (((1ull << k) - 1) & ~255ull) : 0;
  a.loop_mask = all_hi & ~used;
  a.partial = partial;
  const int nbins = 1 << r;
  const unsigned grid = 1u << n_wg;
  double* dev_out = partial + ((u64)grid << 8);
  const bool nt = c->span_bytes > tuning().mall_bytes;
  {
    ProfileScope prof(kClsHist, 16.0 * (double)amps(c), c->stream, nt);
    switch (n_item) {
      case 0: QSIM_WITH_NT(hipLaunchKernelGGL((k_hist<0, NT>), dim3(grid), dim3(kBlock), 0, c->stream, a)); break;
      case 1: QSIM_WITH_NT(hipLaunchKernelGGL((k_hist<1, NT>), dim3(grid), dim3(kBlock), 0, c->stream, a)); break;
      case 2: QSIM_WITH_NT(hipLaunchKernelGGL((k_hist<2, NT>), dim3(grid), dim3(kBlock), 0, c->stream, a)); break;
      default: QSIM_WITH_NT(hipLaunchKernelGGL((k_hist<3, NT>), dim3(grid), dim3(kBlock), 0, c->stream, a)); break;
    }
  }
  HIP_TRY(hipGetLastError());
  if ((rc = sum_rows(c, partial, grid, nbins, dev_out))) return rc;
  return fetch_doubles(c, dev_out, (u64)nbins, out);
}

// Pauli-sum expectation values (expect_kernels.h): the pass plan and the term table on the host (pauli_passes), then
// per pass k_expect_tile (or k_expect_wide) and the rest of pauli_reduce_call, one double per term.
int qsim_plan_expectation(int n_local_qubits, int n_terms, const uint64_t* x_masks, int32_t* pass_of_term, uint64_t* tile_masks, int* n_passes) {
  return plan_pauli_out(false, n_local_qubits, n_terms, x_masks, pass_of_term, tile_masks, n_passes);
}

int qsim_expectation_pauli(qsim_chunk* c, int n_terms, const uint64_t* x_masks, const uint64_t* z_masks, double* out, int* n_passes) {
  int rc = check_pauli_call(c, c, n_terms, x_masks, z_masks, nullptr, nullptr, out, n_passes, "term", "qsim_expectation_pauli");
  if (rc) return rc;
  PauliPasses pp;
  if ((rc = pauli_passes(kPauliExpect, c->k, n_terms, x_masks, z_masks, nullptr, &pp))) return rc;
  *n_passes = 0;
  if (n_terms == 0) return QSIM_OK;
  const bool nt = c->span_bytes > tuning().mall_bytes;
  const auto launch = [&](int q, const PauliTerm* terms, double* partial, unsigned* rows) {
    if (pp.wide_term[(size_t)q] >= 0) {
      const int t = pp.wide_term[(size_t)q];
      ExpWideArgs w;
      std::memset(&w, 0, sizeof w);
      w.amp = c->amp;
      w.partial = partial;
      w.half = amps(c) >> 1;
      w.x = x_masks[t];
      w.z = z_masks[t];
      w.h = 63 - __builtin_clzll(w.x);
      w.cr = pp.entry(pp.first[(size_t)q]).f0;
      w.ci = pp.entry(pp.first[(size_t)q]).f1;
      *rows = pauli_wide_grid(w.half);
      QSIM_WITH_NT(hipLaunchKernelGGL((k_expect_wide<NT>), dim3(*rows), dim3(kBlock), 0, c->stream, w));
    } else {
      ExpArgs a;
      std::memset(&a, 0, sizeof a);
      a.amp = c->amp;
      a.terms = terms;
      a.partial = partial;
      a.w = tile_walk(c->k, pp.plan.tile[(size_t)q]);
      a.n_terms = pp.plan.count[(size_t)q];
      a.slices = pauli_slices(a.n_terms);
      *rows = (unsigned)std::min<u64>(a.w.n_tiles, kExpMaxWg);
      QSIM_WITH_NT(hipLaunchKernelGGL((k_expect_tile<NT>), dim3(*rows), dim3(kBlock), 0, c->stream, a));
    }
    HIP_TRY(hipGetLastError());
    return QSIM_OK;
  };
  return pauli_reduce_call(c, pp, 1, kExpMaxWg, launch, out, n_passes);
}

// Reduced density matrices (rdm_kernels.h, the plans in rdm_plan.h).  Both calls: check, plan, workspace, arguments
// from the plan, one profiled launch, the row sum (k_hist_sum), the copy to the host, the assembly there.
// r <= 6: one read-only pass (k_rdm_small for r <= 3, k_rdm_mfma for r = 4..6), one partial matrix of 4^r doubles per
// workgroup, k_hist_sum over them in workgroup order; the triangle is mirrored on the host (rdm_mirror).  In the
// workspace (ensure_work): at most (kRdmMaxWg + 1) * 4^r doubles, that is 32 MiB +
// 32 KiB at r = 6, 8 MiB at r = 5, 2 MiB at r = 4, 512 KiB at r = 3 (and grid + 1 matrices for chunks of fewer tiles).
int qsim_reduced_density_matrix(qsim_chunk* c, int r, const int32_t* qubits, double* out) {
  int rc = check_chunk(c, "qsim_reduced_density_matrix");
  if (rc) return rc;
  if ((rc = check_qubit_list(c, r, qubits, out, 1, kRdmRowBits, "qsim_reduced_density_matrix"))) return rc;
  RdmPlan p;
  rdm_plan(c->k, r, qubits, &p);
  if ((rc = ensure_work(c, p.work_bytes))) return rc;
  RdmArgs a;
  std::memset(&a, 0, sizeof a);
  rdm_tile_args(p.t, c, &a);
  for (int q = 0; q < r; ++q) a.swz[q] = p.swz[q];
  a.partial = static_cast<double*>(c->work);
  const int dd = 1 << (2 * r);
  double* dev_out = a.partial + (u64)p.grid * dd;
  HIP_TRY(hipSetDevice(c->device));
  const bool nt = c->span_bytes > tuning().mall_bytes;
  {
    ProfileScope prof(kClsRdm, 16.0 * (double)amps(c), c->stream, nt);
#define QSIM_RDM_LAUNCH(KERNEL, R) QSIM_WITH_NT(hipLaunchKernelGGL((KERNEL<R, NT>), dim3(p.grid), dim3(kBlock), 0, c->stream, a));
#ifdef QSIM_PROBES
    if (tuning().rdm_form == 1 && r >= 4) {
      if (r == 4) { QSIM_RDM_LAUNCH(k_rdm_block, 4) } else if (r == 5) { QSIM_RDM_LAUNCH(k_rdm_block, 5) } else { QSIM_RDM_LAUNCH(k_rdm_block, 6) }
    } else
#endif
    switch (r) {
      case 1: QSIM_RDM_LAUNCH(k_rdm_small, 1) break;
      case 2: QSIM_RDM_LAUNCH(k_rdm_small, 2) break;
      case 3: QSIM_RDM_LAUNCH(k_rdm_small, 3) break;
      case 4: QSIM_RDM_LAUNCH(k_rdm_mfma, 4) break;
      case 5: QSIM_RDM_LAUNCH(k_rdm_mfma, 5) break;
      default: QSIM_RDM_LAUNCH(k_rdm_mfma, 6) break;
    }
#undef QSIM_RDM_LAUNCH
  }
  HIP_TRY(hipGetLastError());
  if ((rc = sum_rows(c, a.partial, p.grid, dd, dev_out))) return rc;
  std::vector<double> tri((size_t)dd);
  if ((rc = fetch_doubles(c, dev_out, (u64)dd, tri.data()))) return rc;
  rdm_mirror(r, tri.data(), out);
  return QSIM_OK;
}

// r = 7..12 (k_rdm_wide): one read-only pass of pairs * S workgroups, one partial 64 x 64 block of 64 KiB per
// workgroup, k_hist_sum over the S slices in slice
// order (S = 1: nothing to add), the blocks put together, permuted and mirrored on the host.  In the workspace
// (ensure_work), at most (pairs * S + pairs) blocks with pairs * S <= kRdmWideMaxWg = 2048: 1539 blocks = 96 MiB at
// r = 7, 1290 = 81 MiB at r = 8, 1188 = 74 MiB at r = 9, 1224 = 77 MiB at r = 10, 1584 = 99 MiB at r = 11 and
// 2080 = 130 MiB at r = 12 (S = 1); less for chunks of fewer outer tiles than slices.  2 * 4^r doubles cross to the
// host: 256 KiB at r = 7, 256 MiB at r = 12.
int qsim_reduced_density_matrix_wide(qsim_chunk* c, int r, const int32_t* qubits, double* out) {
  static const char* const what = "qsim_reduced_density_matrix_wide";
  int rc = check_chunk(c, what);
  if (rc) return rc;
  if ((rc = check_qubit_list(c, r, qubits, out, kRdmWideMinQubits, kRdmWideMaxQubits, what, nullptr,
                             " (qsim_reduced_density_matrix serves r <= 6)")))
    return rc;
  RdmWidePlan p;
  rdm_wide_plan(c->k, r, qubits, &p);
  if ((rc = ensure_work(c, p.work_bytes))) return rc;
  RdmWideArgs a;
  std::memset(&a, 0, sizeof a);
  rdm_tile_args(p.t, c, &a);
  for (int b = 0; b < p.nb_bits; ++b) a.blk_phys[b] = p.blk_phys[b];
  a.nb_bits = p.nb_bits;
  a.pairs = p.pairs;
  a.slices = p.slices;
  a.partial = static_cast<double*>(c->work);
  const u64 block_doubles = (u64)p.pairs * kRdmWideBlockDoubles;
  double* dev_out = p.slices > 1 ? a.partial + (u64)p.slices * block_doubles : a.partial;
  HIP_TRY(hipSetDevice(c->device));
  const bool nt = c->span_bytes > tuning().mall_bytes;
  {
    ProfileScope prof(kClsRdmWide, 16.0 * (double)p.nb * (double)amps(c), c->stream, nt);
    QSIM_WITH_NT(hipLaunchKernelGGL((k_rdm_wide<NT>), dim3(p.grid), dim3(kBlock), 0, c->stream, a));
  }
  HIP_TRY(hipGetLastError());
  // k_hist_sum spends a workgroup per output double (4.3 M of them add two rows at r = 11) and also adds the tiles of
  // diagonal partial blocks that no workgroup writes: never-initialised doubles that rdm_wide_assemble does not read
  if (p.slices > 1 && (rc = sum_rows(c, a.partial, p.slices, (int)block_doubles, dev_out))) return rc;
  std::vector<double> blocks;
  try {
    blocks.resize((size_t)block_doubles);          // up to 130 MiB of host memory at r = 12
  } catch (const std::bad_alloc&) {
    return fail(QSIM_ERR_NOMEM, "%s: no host memory for %llu doubles of blocks", what, (u64)block_doubles);
  }
  if ((rc = fetch_doubles(c, dev_out, block_doubles, blocks.data()))) return rc;
  rdm_wide_assemble(p, blocks.data(), out);
  return QSIM_OK;
}

// Shot sampling (sample_kernels.h): pass A (block sums), the block prefix and the shots' blocks on the host, the shots
// grouped by block, pass B (one workgroup per hit block), the indices back in the order of randnums.
int qsim_sample_block_bits(void) { return kSampleBlockBits; }

int qsim_sample_locate(uint64_t n_blocks, const double* block_cdf, uint64_t n_shots, const double* randnums,
                       uint64_t* out_block, double* out_local) {
  if (!n_blocks || !block_cdf || (n_shots && (!randnums || !out_block || !out_local)))
    return fail(QSIM_ERR_INVALID, "qsim_sample_locate: null argument or no blocks");
  if (!(block_cdf[n_blocks - 1] > 0.0) || !std::isfinite(block_cdf[n_blocks - 1]))
    return fail(QSIM_ERR_INVALID, "qsim_sample_locate: the total weight is %g (a positive finite number expected)", block_cdf[n_blocks - 1]);
  for (u64 s = 0; s < n_shots; ++s)
    if (!sample_randnum_ok(randnums[s]))
      return fail(QSIM_ERR_INVALID, "qsim_sample_locate: randnums[%llu] = %g is outside [0, 1)", (u64)s, randnums[s]);
  sample_locate(n_blocks, block_cdf, n_shots, randnums, out_block, out_local);
  return QSIM_OK;
}

int qsim_sample(qsim_chunk* c, uint64_t n_shots, const double* randnums, uint64_t* out_indices, double* total, int* n_passes) {
  int rc = check_chunk(c, "qsim_sample");
  if (rc) return rc;
  if (!total || !n_passes || (n_shots && (!randnums || !out_indices))) return fail(QSIM_ERR_INVALID, "qsim_sample: null argument");
  if (n_shots > kSampleMaxShots) return fail(QSIM_ERR_INVALID, "qsim_sample: %llu shots in one call, at most 2^24", (u64)n_shots);
  if ((rc = require_no_parts(c, "qsim_sample"))) return rc;
  for (u64 s = 0; s < n_shots; ++s)
    if (!sample_randnum_ok(randnums[s]))
      return fail(QSIM_ERR_INVALID, "qsim_sample: randnums[%llu] = %g is outside [0, 1)", (u64)s, randnums[s]);
  *total = 0.0;
  *n_passes = 0;
  if (!n_shots) return QSIM_OK;
  const u64 n = amps(c), n_blocks = std::max<u64>(n >> kSampleBlockBits, 1);
  // device scratch: block sums | shot slots | hit blocks | first shot of every hit block (+ 1)
  const u64 slot_off = sizeof(double) * n_blocks, hit_off = slot_off + sizeof(u64) * n_shots;
  const u64 first_off = hit_off + sizeof(u64) * n_shots;
  if ((rc = ensure_work(c, first_off + sizeof(unsigned) * (n_shots + 1)))) return rc;
  char* base = static_cast<char*>(c->work);
  double* dev_sums = reinterpret_cast<double*>(base);
  u64* dev_slot = reinterpret_cast<u64*>(base + slot_off);
  u64* dev_hit = reinterpret_cast<u64*>(base + hit_off);
  unsigned* dev_first = reinterpret_cast<unsigned*>(base + first_off);
  HIP_TRY(hipSetDevice(c->device));
  const bool nt = c->span_bytes > tuning().mall_bytes;
  {
    ProfileScope prof(kClsSampleSums, 16.0 * (double)n, c->stream, nt);
    QSIM_WITH_NT(hipLaunchKernelGGL((k_sample_block_sums<NT>), grid_for(n_blocks), dim3(kBlock), 0, c->stream, (const double2*)c->amp, n, n_blocks, dev_sums));
  }
  HIP_TRY(hipGetLastError());
  std::vector<double> cdf(n_blocks);
  if ((rc = fetch_doubles(c, dev_sums, n_blocks, cdf.data()))) return rc;
  *n_passes = 1;
  long double run = 0;                               // the block prefix, in block order (rounding to double keeps it monotone)
  for (u64 b = 0; b < n_blocks; ++b) { run += cdf[b]; cdf[b] = (double)run; }
  *total = cdf[n_blocks - 1];
  if (!(*total > 0.0) || !std::isfinite(*total)) return fail(QSIM_ERR_INVALID, "qsim_sample: sum |amp|^2 = %g, nothing to sample from", *total);
  std::vector<uint64_t> block(n_shots);
  std::vector<double> local(n_shots);
  sample_locate(n_blocks, cdf.data(), n_shots, randnums, block.data(), local.data());
  std::vector<unsigned> order(n_shots);              // the shots grouped by block (ties in the order of randnums)
  for (u64 s = 0; s < n_shots; ++s) order[s] = (unsigned)s;
  std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return block[a] != block[b] ? block[a] < block[b] : a < b; });
  std::vector<u64> slot(n_shots), hit;
  std::vector<unsigned> first;
  for (u64 j = 0; j < n_shots; ++j) {
    const unsigned s = order[j];
    if (!j || block[s] != hit.back()) { hit.push_back(block[s]); first.push_back((unsigned)j); }
    std::memcpy(&slot[j], &local[s], sizeof(double));
  }
  first.push_back((unsigned)n_shots);
  const u64 n_hit = hit.size();
  HIP_TRY(hipMemcpyAsync(dev_slot, slot.data(), sizeof(u64) * n_shots, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dev_hit, hit.data(), sizeof(u64) * n_hit, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dev_first, first.data(), sizeof(unsigned) * (n_hit + 1), hipMemcpyHostToDevice, c->stream));
  {
    ProfileScope prof(kClsSampleResolve, 16.0 * (double)std::min<u64>(n, n_hit << kSampleBlockBits), c->stream, nt);
    QSIM_WITH_NT(hipLaunchKernelGGL((k_sample_resolve<NT>), grid_for(n_hit), dim3(kBlock), 0, c->stream, (const double2*)c->amp, n, n_blocks, (const u64*)dev_hit, (const unsigned*)dev_first, n_hit, dev_slot));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(slot.data(), dev_slot, sizeof(u64) * n_shots, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (u64 j = 0; j < n_shots; ++j) out_indices[order[j]] = slot[j];
  *n_passes = 2;
  return QSIM_OK;
}

// Sparse export: the amplitudes with |re| > eps or |im| > eps as rows (index, re, im), ascending by index.
int qsim_count_nonzero(qsim_chunk* c, double eps, uint64_t* count) {
  int rc = check_chunk(c, "qsim_count_nonzero");
  if (rc) return rc;
  if (!count || !(eps >= 0)) return fail(QSIM_ERR_INVALID, "qsim_count_nonzero: bad arguments");
  if ((rc = ensure_scratch(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long* dcount = reinterpret_cast<unsigned long long*>(c->scratch);
  HIP_TRY(hipMemsetAsync(dcount, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_count_kept, dim3(stream_grid(amps(c))), dim3(kBlock), 0, c->stream, c->amp, amps(c), eps, dcount);
  HIP_TRY(hipGetLastError());
  unsigned long long host = 0;
  HIP_TRY(hipMemcpyAsync(&host, dcount, sizeof host, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *count = host;
  return QSIM_OK;
}

int qsim_export_nonzero(qsim_chunk* c, double eps, uint64_t capacity, uint64_t* out_idx, double* out_re_im, uint64_t* n_rows) {
  int rc = check_chunk(c, "qsim_export_nonzero");
  if (rc) return rc;
  if (!n_rows || !(eps >= 0) || (capacity && (!out_idx || !out_re_im))) return fail(QSIM_ERR_INVALID, "qsim_export_nonzero: bad arguments");
  if ((rc = ensure_scratch(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  u64* didx = nullptr;
  double2* damp = nullptr;
  if (capacity) {
    if (hipMalloc((void**)&didx, sizeof(u64) * capacity) != hipSuccess) return fail(QSIM_ERR_NOMEM, "qsim_export_nonzero: no device memory for %llu rows", (u64)capacity);
    if (hipMalloc((void**)&damp, sizeof(double2) * capacity) != hipSuccess) { (void)hipFree(didx); return fail(QSIM_ERR_NOMEM, "qsim_export_nonzero: no device memory for %llu rows", (u64)capacity); }
  }
  unsigned long long* cursor = reinterpret_cast<unsigned long long*>(c->scratch);
  auto cleanup = [&]() { if (didx) (void)hipFree(didx); if (damp) (void)hipFree(damp); };
  hipError_t e = hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_append_kept, dim3(stream_grid(amps(c))), dim3(kBlock), 0, c->stream, c->amp, amps(c), eps, cursor, (u64)capacity, didx, damp);
    e = hipGetLastError();
  }
  unsigned long long total = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&total, cursor, sizeof total, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  const u64 got = std::min<u64>(total, capacity);
  std::vector<u64> idx(got);
  std::vector<double2> amp(got);
  if (e == hipSuccess && got) e = hipMemcpy(idx.data(), didx, sizeof(u64) * got, hipMemcpyDeviceToHost);
  if (e == hipSuccess && got) e = hipMemcpy(amp.data(), damp, sizeof(double2) * got, hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return fail(QSIM_ERR_HIP, "qsim_export_nonzero: %s", hipGetErrorString(e));
  *n_rows = total;
  if (total > capacity) return QSIM_OK;             // the caller sees n_rows > capacity and comes back with room (nothing written)
  std::vector<u64> order(got);
  for (u64 i = 0; i < got; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](u64 a, u64 b) { return idx[a] < idx[b]; });
  for (u64 i = 0; i < got; ++i) {
    out_idx[i] = idx[order[i]];
    out_re_im[2 * i] = amp[order[i]].x;
    out_re_im[2 * i + 1] = amp[order[i]].y;
  }
  return QSIM_OK;
}

static int bit_perm_from(const int32_t* log_to_phys, int n_total_qubits, BitPerm* perm, const char* what) {
  std::memset(perm, 0, sizeof *perm);
  if (!log_to_phys) return QSIM_OK;
  u64 seen = 0;
  for (int q = 0; q < n_total_qubits; ++q) {
    const int ph = log_to_phys[q];
    if (ph < 0 || ph >= n_total_qubits || (seen >> ph) & 1) return fail(QSIM_ERR_INVALID, "%s: log_to_phys is not a permutation", what);
    seen |= 1ull << ph;
    perm->to_logical[ph] = (unsigned char)q;
    if (ph != q) perm->active = 1;
  }
  return QSIM_OK;
}

int qsim_max_abs_err_closed_form(qsim_chunk* c, int kind, int n_total_qubits, uint64_t base_index, double* out) {
  return qsim_max_abs_err_closed_form_perm(c, kind, n_total_qubits, base_index, nullptr, out);
}

int qsim_max_abs_err_closed_form_perm(qsim_chunk* c, int kind, int n_total_qubits, uint64_t base_index, const int32_t* log_to_phys, double* out) {
  int rc = check_chunk(c, "qsim_max_abs_err_closed_form");
  if (rc) return rc;
  if (!out || (kind != 0 && kind != 1) || n_total_qubits < c->k || n_total_qubits > 52)
    return fail(QSIM_ERR_INVALID, "qsim_max_abs_err_closed_form: bad arguments");
  if (base_index & (amps(c) - 1)) return fail(QSIM_ERR_INVALID, "qsim_max_abs_err_closed_form: base_index must be a multiple of the chunk length");
  if ((base_index + amps(c) - 1) >> n_total_qubits) return fail(QSIM_ERR_INVALID, "qsim_max_abs_err_closed_form: the chunk does not fit a state of %d qubits at that base", n_total_qubits);
  BitPerm perm;
  if ((rc = bit_perm_from(log_to_phys, n_total_qubits, &perm, "qsim_max_abs_err_closed_form"))) return rc;
  if ((rc = ensure_scratch(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const unsigned grid = std::min<unsigned>(stream_grid(amps(c)), kReduceBlocks);
  hipLaunchKernelGGL(k_closed_form_err, dim3(grid), dim3(kBlock), 0, c->stream, c->amp, amps(c), kind,
                     n_total_qubits, (u64)base_index, c->scratch, perm);
  HIP_TRY(hipGetLastError());
  return reduce_partials(c, grid, 1, true, out);
}

// sum over the chunk's amplitudes whose logical index passes the filter of amp * w(logical index): see k_fingerprint
int qsim_fingerprint(qsim_chunk* c, int n_total_qubits, uint64_t base_index, const int32_t* log_to_phys, uint64_t seed,
                     uint64_t sel_mask, uint64_t sel_value, double out[2]) {
  int rc = check_chunk(c, "qsim_fingerprint");
  if (rc) return rc;
  if (!out || n_total_qubits < c->k || n_total_qubits > 52) return fail(QSIM_ERR_INVALID, "qsim_fingerprint: bad arguments");
  if (base_index & (amps(c) - 1)) return fail(QSIM_ERR_INVALID, "qsim_fingerprint: base_index must be a multiple of the chunk length");
  if (n_total_qubits < 64 && ((base_index + amps(c) - 1) >> n_total_qubits)) return fail(QSIM_ERR_INVALID, "qsim_fingerprint: the chunk does not fit a state of %d qubits at that base", n_total_qubits);
  if (sel_value & ~sel_mask) return fail(QSIM_ERR_INVALID, "qsim_fingerprint: sel_value has bits outside sel_mask");
  BitPerm perm;
  if ((rc = bit_perm_from(log_to_phys, n_total_qubits, &perm, "qsim_fingerprint"))) return rc;
  if ((rc = ensure_scratch(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const unsigned grid = std::min<unsigned>(stream_grid(amps(c)), kReduceBlocks / 2);
  hipLaunchKernelGGL(k_fingerprint, dim3(grid), dim3(kBlock), 0, c->stream, c->amp, amps(c), n_total_qubits, (u64)base_index,
                     fp_mix((u64)seed), (u64)sel_mask, (u64)sel_value, c->scratch, perm);
  HIP_TRY(hipGetLastError());
  return reduce_partials(c, grid, 2, false, out);
}
}  // extern "C"
