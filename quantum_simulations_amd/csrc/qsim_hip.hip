// libqsim_hip.so -- gate-application kernels for MI355X (gfx950 / CDNA4), C ABI in
// include/qsim_hip.h.  Written for wave64, 16-byte (complex128) lane accesses and the
// HBM roofline: every gate is a streaming read-modify-write of the amplitudes it touches.
//
// Kernel family (one template, `k_gate<NM, ITEMS>`):
//   a gate is reduced on the host to
//     * a sorted list of index bit positions that are *removed* from the work-item
//       index (target bits and fixed-one control/diagonal bits),
//     * NM = 1, 2 or 4 "member" base pointers (the NM amplitudes one work item owns:
//       target-bit combinations, with fixed-one bits and partner-chunk selection folded
//       into the pointer),
//     * an NM x NM complex matrix.
//   NM=1: x *= d           diagonal Z/S/T/R (half the state), CZ/CR (a quarter)
//   NM=2: 2x2 butterfly    dense 1q, controlled-1q (CNOT/CY/CU: half), SWAP (half),
//                          apply_1q_pair across two chunks
//   NM=4: 4x4 butterfly    dense 2q, partner-chunk pair/quad forms
//   Each amplitude belongs to exactly one work item, so the update is in place with
//   no inter-thread hazard.  Lanes own consecutive work items => a wave's 16-B loads
//   cover contiguous runs of 2^(lowest removed bit) amplitudes (1 KiB when that bit >= 6).
//
// Algorithmic HBM bytes per launch: 32 * NM * count (read + write of every member).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/qsim_hip.h"

typedef unsigned long long u64;

// The sources are split by topic and compiled as ONE translation unit (kernels, their launchers and
// the C ABI share file-local state; hipcc needs no relocatable device code this way).
#include "qsim_core.h"
#include "gate_kernels.h"
#include "gate_plan.h"
#include "tile_kernel.h"
// the host planner of the fused passes (no device call in any of these), then what launches its passes
#include "tile_ops.h"
#include "tile_groups.h"
#include "tile_planner.h"
#include "tile_search.h"
#include "op_rewrite.h"
#include "tile_launch.h"
#include "state_kernels.h"
#include "readout_kernels.h"
#include "dense_kernels.h"
// pauli_tile.h first: the tile walk, the term record and the plan that the four Pauli-string families below share
// (rdm_kernels.h takes its tile_base from it too)
#include "pauli_tile.h"
#include "expect_kernels.h"
#include "rot_kernels.h"
#include "diag_plan.h"
#include "diag_kernels.h"
#include "psum_kernels.h"
#include "ovl_kernels.h"
#include "lincomb_kernels.h"
#include "rdm_plan.h"
#include "rdm_kernels.h"
#include "sample_kernels.h"
#include "comm_rccl.h"

// The C ABI, by topic.  abi_pending.h first: every topic asks whether a split call has left pieces pending on a chunk.
#include "abi_pending.h"
#include "abi_readout.h"
#include "abi_rotation.h"
#include "abi_diagonal.h"
#include "abi_twostate.h"
#include "abi_lincomb.h"
#include "abi_chunk.h"
#include "abi_gates.h"
#include "abi_plan.h"
#include "abi_relayout.h"
#include "abi_comm.h"
