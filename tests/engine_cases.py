"""Directed op lists for the branch table of the fused-pass gate engine (test infrastructure, no GPU needed).

The engine (csrc/gen_tile_engine.py -> tile_engine_gen.h) is a direct-threaded interpreter: every gate record jumps
to one CASE of a branch table -- a family (OPC_DENSE1, OPC_PHASE, ...) plus a variant (target / control register,
register mask) -- either directly or, for a predicated gate, through a second dispatch (OPC_PRED_LANE,
OPC_PRED_OUTER, OPC_PRED_OUTER_ZERO).  It exists in two generated texts: FULL (tiles of 2^11 amplitudes, chunks of
11 or more qubits) and PARTIAL (tiles of 2^8..2^10 amplitudes, chunks of 8 to 10 qubits).  Every case is its own
stretch of assembly, so a mistake in one case only shows on gates that land on it.

This module builds, for every (engine text, family, variant, predicate form) the planner can emit, one short op list
that makes the planner emit exactly that (`directed_lists`), reads back what a planned list really contains
(`ledger`), names what the planner can never emit (`UNREACHABLE`, `possible_forms`) and states the operation a second
time in extended precision (`reference`).  tests/test_engine_case_ledger.py proves the coverage on the CPU;
tests/test_gpu_engine_cases.py runs every list on the device.  `paired_lists` are the FULL lists once more at 24 qubits,
where a workgroup takes two tiles (tests/test_gpu_engine_cases_paired.py).

How a list is aimed (csrc/tile_planner.h, csrc/tile_groups.h).  The lists are short and every target is an index bit below 11, so a
chunk of n qubits is planned as ONE pass whose tile bits are the index bits 0..T-1, T = min(n, 11) (plan_fused fills
the tile "with the lowest unused bits"); tile position = qubit.  Qubits >= 11 of a 14-qubit chunk lie outside the
tile.  The ops of a list target at most three distinct bits, so the pass has one register group: the targeted bits,
padded "with the highest unused tile bits" (GroupEmitter::write_group).  Two layouts are used:
  * HI : registers (r0, r1, r2) = tile bits (T-3, T-2, T-1) -- every target is one of them;
  * LOW: registers = tile bits (0, T-2, T-1) -- one op targets bit 0.  A full tile whose last group lies above the
    line bits is stored without a write-back, where serialize_pass turns OPC_ASWAP1 back into OPC_SWAP1, so the FULL
    lists for OPC_ASWAP1 use LOW.
A control or phase bit on a register bit selects the variant, on another tile bit (3, 4) it becomes a lane
predicate, outside the tile (12, 13) an outer predicate (require_one).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import tile_interpreter as ti

FULL, PARTIAL = "FULL", "PARTIAL"
FORMS = ("none", "lane", "outer", "lane+outer", "outer-zero")
PARTIAL_SIZES = (8, 9, 10)
FULL_SIZES = (11, 14)          # one tile; 8 tiles with three index bits outside the tile
FAMILIES = ti._FAMILIES
WIDTH = ti.FAMILY_WIDTH        # variants per family: the engine's branch table

_1Q_CONTROLLED = ("DENSE1", "SWAP1", "ANTI1", "REAL1", "YLIKE1", "ASWAP1")   # families of a 1q gate with an optional control
_ZERO_FAMILIES = ("DENSE1", "REAL1", "ANTI1", "YLIKE1")
_PHASES = ("PHASE", "PHASE_NEG", "PHASE_I", "PHASE_NI")

# Entries of the table the planner never emits: (family, variant, the line of csrc/tile_ops.h / tile_groups.h that rules it out, why).
_L_DENSE2 = "d.opcode = (uint8_t)(OPC_DENSE2 + 3 * reg_pos(tile_pos(o.target[0])) + reg_pos(tile_pos(o.target[1])));"
_W_DENSE2 = "the two targets of an op are distinct qubits, hence distinct registers: JA != JB, never 3 * J + J"
_L_HAD1 = "if (sp && tuning().tile_had && o.control < 0 && o.m[0].y == 0 && o.m[1].y == 0 && o.m[2].y == 0 && o.m[3].y == 0 &&"
_W_HAD1 = "op_shape gives OPC_HAD1 to an uncontrolled gate only, and opc_1q_variant(J, -1) = J < 3"
_L_MASK7 = "int bits[2]; // TG_PHASE: qubits that must be 1"
_W_MASK7 = "an op has at most two phase bits and a merged run is written out one register bit at a time: never all three"
UNREACHABLE = (
    [("DENSE2", v, _L_DENSE2, _W_DENSE2) for v in (0, 4, 8)]
    + [("HAD1", v, _L_HAD1, _W_HAD1) for v in range(3, 9)]
    + [(f, 7, _L_MASK7, _W_MASK7) for f in _PHASES]
)
_UNREACHABLE_SET = {(f, v) for f, v, _, _ in UNREACHABLE}


def table() -> set:
    """Every (family, variant) of the branch table."""
    return {(f, v) for f in FAMILIES for v in range(WIDTH[f])}


def possible_forms(text: str, family: str, variant: int) -> tuple:
    """Predicate forms the planner can give an entry in one engine text.  Outer forms need index bits outside the
    tile: FULL only.  Reasons (csrc/tile_groups.h, GroupEmitter::describe and mux_pairs):
      * a 1q gate has ONE control (FusedOp::control): on a register it selects variants 3..8 (no predicate left), else it
        is a lane OR an outer predicate -- never both;
      * OPC_PRED_OUTER_ZERO is the control = 0 half of the tile_mux pair, whose U satisfies is_plain_1q (kind TG_DENSE1
        or TG_ANTI1, no control of its own): DENSE1 / REAL1 / ANTI1 / YLIKE1, variants 0..2;
      * a phase op has one or two bits: two register bits leave no predicate, one leaves one bit, and mask 0 has every
        bit in the predicate -- it is never unpredicated;
      * OPC_DIAGR merges phases with ONE register bit each and the same predicate: at most one other bit;
      * OPC_DENSE2, OPC_HAD1 (uncontrolled by op_shape) and OPC_SCALE get no predicate at all."""
    outer = text == FULL
    if (family, variant) in _UNREACHABLE_SET:
        return ()
    if family in _1Q_CONTROLLED:
        if variant >= 3:
            return ("none",)
        forms = ["none", "lane"] + (["outer"] if outer else [])
        if outer and family in _ZERO_FAMILIES:
            forms.append("outer-zero")
        return tuple(forms)
    if family in _PHASES:
        bits = bin(variant).count("1")
        if bits == 2:
            return ("none",)
        if bits == 1:
            return ("none", "lane") + (("outer",) if outer else ())
        return ("lane",) + (("outer", "lane+outer") if outer else ())
    if family == "DIAGR":
        return ("none", "lane") + (("outer",) if outer else ())
    return ("none",)


def required(text: str) -> set:
    """Every (family, variant, form) a directed list has to reach in one engine text."""
    return {(f, v, form) for f, v in table() for form in possible_forms(text, f, v)}


# ---------------------------------------------------------------------------------------------------------------------
# matrices: every entry a record carries has its own value, |entries| <= 1 (the engine does not need unitarity)
M_DENSE = np.array([[0.31 + 0.52j, -0.44 + 0.27j], [0.63 - 0.19j, 0.12 + 0.71j]])
M_DENSE_B = np.array([[-0.22 + 0.41j, 0.57 + 0.33j], [0.18 - 0.64j, -0.49 - 0.28j]])   # the V of a tile_mux pair
M_REAL = np.array([[0.35, -0.62], [0.81, 0.47]], dtype=complex)      # not a rotation: r00 != r11, r01 != -r10
M_ANTI = np.array([[0, 0.58 - 0.41j], [-0.23 + 0.77j, 0]])           # u01 != u10
M_X = np.array([[0, 1], [1, 0]], dtype=complex)
M_Y = np.array([[0, -1j], [1j, 0]])
M_HAD = 0.6 * np.array([[1, 1], [1, -1]], dtype=complex)             # c [[1,1],[1,-1]] with c != 1/sqrt(2)
M_HAD_B = -0.85 * np.array([[1, 1], [1, -1]], dtype=complex)
P_GENERIC = 0.9 * np.exp(0.9j)                                         # well away from +-1 and +-i
P_RUN = (0.95 * np.exp(0.7j), 0.85 * np.exp(-1.9j), 0.9 * np.exp(2.6j))   # three distinct phases of a merged run
P_COMPANION = 0.8 * np.exp(-2.3j)
_PHASE_VALUE = {"PHASE": P_GENERIC, "PHASE_NEG": -1.0, "PHASE_I": 1j, "PHASE_NI": -1j}
_MATRIX_1Q = {"DENSE1": M_DENSE, "SWAP1": M_X, "ANTI1": M_ANTI, "REAL1": M_REAL, "YLIKE1": M_Y, "ASWAP1": M_X, "HAD1": M_HAD}


def _dense4(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (4, 4)) + 1j * rng.uniform(-0.5, 0.5, (4, 4))   # 32 distinct doubles, |entry| < 0.71


def phase1(q: int, p: complex):
    return ([q], np.diag([1, p]).astype(complex))


def cphase(qa: int, qb: int, p: complex):
    return ([qa, qb], np.diag([1, 1, 1, p]).astype(complex))


def controlled(control: int, target: int, M: np.ndarray, control_first: bool):
    """C(M) as a 4x4 on (control, target) or on (target, control): a 2q matrix is big-endian inside its pair."""
    U = np.eye(4, dtype=complex)
    if control_first:
        U[2:, 2:] = M
        return ([control, target], U)
    U[np.ix_([1, 3], [1, 3])] = M
    return ([target, control], U)


Case = namedtuple("Case", "text n family variant form ops note")


def case_id(c: Case) -> str:
    return f"{c.text}-n{c.n}-{c.family}+{c.variant}-{c.form}" + (f"-{c.note}" if c.note else "")


def variant_registers(variant: int):
    """1q variant -> (target register, control register or None): opc_1q_variant of csrc/tile_kernel.h."""
    if variant < 3:
        return variant, None
    J, k = (variant - 3) // 2, (variant - 3) % 2
    return J, [r for r in range(3) if r != J][k]


class _Geometry:
    def __init__(self, n: int, outer=None):
        self.n = n
        self.T = min(n, 11)
        self.text = FULL if self.T == 11 else PARTIAL
        self.hi = (self.T - 3, self.T - 2, self.T - 1)
        self.low = (0, self.T - 2, self.T - 1)
        self.lane = (3, 4)                                  # tile bits that are no register bits (T - 3 >= 5)
        # index bits outside the tile (a pair; which of the two a list uses follows its variant)
        self.outer = tuple(outer) if outer is not None else (12, 13) if n >= 14 else None
        assert self.outer is None or (len(set(self.outer)) == 2 and all(self.T <= b < n for b in self.outer))


def _lists_1q(g: _Geometry, family: str):
    M = _MATRIX_1Q[family]
    for variant in range(WIDTH[family]):
        for form in possible_forms(g.text, family, variant):
            if form in ("outer", "outer-zero") and g.outer is None:
                continue
            J, C = variant_registers(variant)
            # (see the module docstring: a sunk swap only survives in a full tile when its group has a write-back)
            low = family == "ASWAP1" and g.T == 11
            regs = g.low if low else g.hi
            t = regs[J]
            if low and J != 0:
                companion = ([0], M_DENSE)                   # claims tile bit 0 for the group
            else:
                free = next(r for r in range(3) if r not in (J, C) and not (low and r == 0))
                companion = phase1(regs[free], P_COMPANION)
            ops = []
            if form == "none":
                gate = ([t], M) if C is None else controlled(regs[C], t, M, control_first=variant % 2 == 1)
            elif form == "lane":
                gate = controlled(g.lane[variant % 2], t, M, control_first=variant % 2 == 0)
            elif form == "outer":
                gate = controlled(g.outer[variant % 2], t, M, control_first=variant % 2 == 1)
            else:   # outer-zero: C(V) with its control outside the tile, then the plain 1q gate U on its target (tile_mux)
                ops.append(companion)
                ops.append(controlled(g.outer[variant % 2], t, M_DENSE_B, control_first=variant % 2 == 0))
                ops.append(([t], M))
                yield Case(g.text, g.n, family, variant, form, ops, "")
                continue
            if family == "SWAP1":
                # something later in the group touches the target: the swap cannot sink into the write-back
                ops += [gate, cphase(t, regs[free], P_COMPANION)]
            else:
                # (OPC_HAD1: no plain dense / real / anti-diagonal gate to fold the factor into -- it goes into OPC_SCALE)
                ops += [companion, gate]
            yield Case(g.text, g.n, family, variant, form, ops, "")


def _lists_phase(g: _Geometry, family: str):
    p = _PHASE_VALUE[family]
    regs = g.hi
    for variant in range(WIDTH[family]):
        on = [r for r in range(3) if (variant >> r) & 1]
        free = [r for r in range(3) if r not in on]
        for form in possible_forms(g.text, family, variant):
            if "outer" in form and g.outer is None:
                continue
            ops = [([regs[free[-1]]], M_REAL)]              # a second op on a register the phase does not use
            if len(on) == 2:
                ops.append(cphase(regs[on[0]], regs[on[1]], p))
            elif len(on) == 1:
                other = {"lane": g.lane[variant % 2], "outer": g.outer and g.outer[variant % 2]}.get(form)
                ops.append(phase1(regs[on[0]], p) if form == "none" else
                           cphase(regs[on[0]], other, p) if variant & 2 else cphase(other, regs[on[0]], p))
            elif form == "lane":
                ops.append(cphase(g.lane[0], g.lane[1], p))
            elif form == "outer":
                ops.append(cphase(g.outer[1], g.outer[0], p))
            else:
                ops.append(cphase(g.lane[1], g.outer[0], p))
            yield Case(g.text, g.n, family, variant, form, ops, "")
    # mask 0 again, from a ONE-bit phase on a tile bit outside the registers (on an index bit outside the tile)
    yield Case(g.text, g.n, family, 0, "lane", [([regs[2]], M_REAL), phase1(g.lane[1], p)], "1bit")
    if g.outer is not None:
        yield Case(g.text, g.n, family, 0, "outer", [([regs[2]], M_REAL), phase1(g.outer[0], p)], "1bit")


def _lists_diagr(g: _Geometry):
    regs = g.hi
    for variant, on in enumerate(((0, 1), (0, 2), (1, 2), (0, 1, 2))):
        free = [r for r in range(3) if r not in on]
        for form in possible_forms(g.text, "DIAGR", variant):
            if form == "outer" and g.outer is None:
                continue
            ops = [([regs[free[0]]], M_REAL)] if free else []
            for e, r in enumerate(on):                       # phases that share their predicate, one per register bit
                if form == "none":
                    ops.append(phase1(regs[r], P_RUN[e]))
                else:
                    other = g.lane[variant % 2] if form == "lane" else g.outer[variant % 2]
                    ops.append(cphase(regs[r], other, P_RUN[e]) if e % 2 else cphase(other, regs[r], P_RUN[e]))
            yield Case(g.text, g.n, "DIAGR", variant, form, ops, "")


def _lists_dense2(g: _Geometry):
    regs = g.hi
    for variant in range(WIDTH["DENSE2"]):
        if not possible_forms(g.text, "DENSE2", variant):
            continue
        JA, JB = variant // 3, variant % 3
        free = next(r for r in range(3) if r not in (JA, JB))
        yield Case(g.text, g.n, "DENSE2", variant, "none",
                   [phase1(regs[free], P_COMPANION), ([regs[JA], regs[JB]], _dense4(40 + variant))], "")


def _lists_scale(g: _Geometry):
    # two Hadamard-like gates, nothing to fold the product of their factors into
    yield Case(g.text, g.n, "SCALE", 0, "none", [([g.hi[0]], M_HAD), ([g.hi[2]], M_HAD_B)], "")
    # (control: WITH a plain dense gate in the pass the factor is folded into its matrix -- no OPC_SCALE record)
    yield Case(g.text, g.n, "HAD1", 1, "none", [([g.hi[0]], M_DENSE), ([g.hi[1]], M_HAD)], "folded")


def _lists_layout(g: _Geometry):
    """Full tiles: a pass whose first (last) register group lies above the line bits loads (stores) the tile in that
    group's layout (OPC_GROUP_DIRECT / OPC_END_DIRECT).  The HI lists are direct on both ends and the LOW lists on
    neither; these two have two groups, one above the line bits and one on tile bit 0."""
    a, b, c = g.hi
    # the group on bit 0 shares qubit a with the one before it: it stays last -- direct in, write-back at the end
    yield Case(g.text, g.n, "DENSE1", 0, "lane", [([a], M_DENSE), ([b], M_REAL), ([c], M_ANTI),
                                                  controlled(a, 0, M_DENSE_B, True)], "direct-in")
    # groups on disjoint qubits commute: the one on bit 0 is moved to the front -- LDS read first, direct out
    yield Case(g.text, g.n, "REAL1", 0, "none", [([0], M_REAL), ([a], M_DENSE), ([b], M_DENSE_B), ([c], M_ANTI)], "direct-out")


def _lists_of(g: _Geometry) -> list:
    out = []
    for family in FAMILIES:
        if family in _1Q_CONTROLLED or family == "HAD1":
            out += list(_lists_1q(g, family))
        elif family in _PHASES:
            out += list(_lists_phase(g, family))
        elif family == "DIAGR":
            out += list(_lists_diagr(g))
        elif family == "DENSE2":
            out += list(_lists_dense2(g))
        else:
            out += list(_lists_scale(g))
    if g.text == FULL:
        out += list(_lists_layout(g))
    return out


def directed_lists() -> list:
    """Every directed list, in a fixed order: [Case(text, n, family, variant, form, ops, note)].  A case is AIMED at its
    (family, variant, form); `ledger` tells what its plan really holds."""
    out = []
    for n in PARTIAL_SIZES + FULL_SIZES:
        out += _lists_of(_Geometry(n))
    ids = [case_id(c) for c in out]
    assert len(set(ids)) == len(ids)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The FULL lists once more where a workgroup of k_tile takes TWO tiles (csrc/tile_launch.h: from 2 x 4096 tiles on, i.e.
# 24 qubits with 11-bit tiles; planner.tiles_per_workgroup).  The tile is still index bits 0..10, so the tile number is
# index >> 11 and the two tiles of a workgroup (tile numbers 2w, 2w + 1) differ in index bit 11 alone.  The outer pair is
# (11, 23): an outer predicate on bit 11 differs INSIDE a tile pair (the engine's `baseh` has to be the one of the tile it
# works on), one on bit 23 differs across the grid.  Which of the pair a list uses follows its variant, so the lists with
# an outer predicate are built with both orders of the pair: each sees its predicate at either place.
PAIRED_N = 24
PAIRED_OUTER = (11, 23)
PAIRED_ACTIVE = 13             # the lists touch index bits 0..11 and 23 only: 13 "active" qubits, bits 12..22 look on


def outer_bits(c: Case) -> tuple:
    """Index bits outside the (11-bit) tile a list touches, in the order of their first appearance."""
    seen = []
    for qubits, _ in c.ops:
        seen += [q for q in qubits if q >= 11 and q not in seen]
    return tuple(seen)


def paired_lists() -> list:
    """The FULL directed lists at PAIRED_N qubits, in a fixed order: all of them with the outer pair (11, 23), then those
    whose form has an outer predicate with (23, 11).  The note of a list that touches a bit outside the tile ends in
    o<bits>, e.g. o11, o23 or o23.11 (in order of appearance): the ids are unique and name the placement."""
    def tagged(g, keep):
        for c in _lists_of(g):
            if keep(c):
                bits = ".".join(str(b) for b in outer_bits(c))
                yield c._replace(note="-".join(x for x in (c.note, "o" + bits if bits else "") if x))
    out = list(tagged(_Geometry(PAIRED_N, PAIRED_OUTER), lambda c: True))
    out += list(tagged(_Geometry(PAIRED_N, PAIRED_OUTER[::-1]), lambda c: "outer" in c.form))
    ids = [case_id(c) for c in out]
    assert len(set(ids)) == len(ids)
    return out


def to_active(ops) -> list:
    """A paired list on its 13-qubit active register: index bit 23 relabelled 12 (bits 12..22 are untouched)."""
    assert all(q <= 11 or q == 23 for qubits, _ in ops for q in qubits)
    return [([12 if q == 23 else q for q in qubits], U) for qubits, U in ops]


# ---------------------------------------------------------------------------------------------------------------------
def ledger_of_images(images) -> set:
    """{(engine text, family, variant, predicate form)} of the gate records of planned pass images."""
    seen = set()
    for img in images:
        text = FULL if int(img["T"]) == 11 else PARTIAL
        for rec in ti.records(img):
            if rec[0] != "gate":
                continue
            _, case, blk, outer = rec[:4]
            family = ti.fam_of(case)
            form = ("lane+outer" if blk and outer else "lane" if blk else "outer-zero" if outer < 0 else "outer" if outer else "none")
            assert not (blk and outer < 0)
            seen.add((text, family, case - ti.OPC[family], form))
    return seen


def ledger(n_qubits: int, ops) -> set:
    return ledger_of_images(ti.plan(n_qubits, ops))


def outer_masks_of_images(images) -> set:
    """{(family, variant, predicate form, outer mask)} of the predicated gate records with index bits outside the tile:
    the mask holds the absolute index bits that must be 1 (for outer-zero: that must be 0)."""
    seen = set()
    for img in images:
        for rec in ti.records(img):
            if rec[0] == "gate" and rec[3]:
                _, case, blk, outer = rec[:4]
                family = ti.fam_of(case)
                form = "lane+outer" if blk else "outer-zero" if outer < 0 else "outer"
                seen.add((family, case - ti.OPC[family], form, abs(outer)))
    return seen


def direct_flags(images) -> set:
    """{(direct in, direct out)} of planned pass images."""
    return {(bool(int(img["order"]) & ti.DIRECT_IN), bool(int(img["order"]) & ti.DIRECT_OUT)) for img in images}


# ---------------------------------------------------------------------------------------------------------------------
# The operation once more, in extended precision: butterflies gate by gate in list order, by the conventions of the
# C ABI (include/qsim_hip.h): qubit q is index bit q; a 2q matrix acts on the pair index 2 * bit(qa) + bit(qb).
def random_state(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (v / np.linalg.norm(v)).astype(np.complex128)


def reference(psi: np.ndarray, ops) -> np.ndarray:
    """The state after `ops`, computed in np.clongdouble (returned as such)."""
    n = int(psi.size).bit_length() - 1
    out = psi.astype(np.clongdouble)
    for qubits, U in ops:
        U = np.asarray(U).astype(np.clongdouble)
        if len(qubits) == 1:
            v = out.reshape(1 << (n - 1 - qubits[0]), 2, 1 << qubits[0])
            lo, hi = v[:, 0, :].copy(), v[:, 1, :].copy()
            v[:, 0, :] = U[0, 0] * lo + U[0, 1] * hi
            v[:, 1, :] = U[1, 0] * lo + U[1, 1] * hi
        else:
            qa, qb = qubits
            idx = np.arange(psi.size)
            base = idx[((idx >> qa) & 1 == 0) & ((idx >> qb) & 1 == 0)]
            at = [base, base | (1 << qb), base | (1 << qa), base | (1 << qa) | (1 << qb)]
            old = [out[i].copy() for i in at]
            for r in range(4):
                out[at[r]] = U[r, 0] * old[0] + U[r, 1] * old[1] + U[r, 2] * old[2] + U[r, 3] * old[3]
    return out
