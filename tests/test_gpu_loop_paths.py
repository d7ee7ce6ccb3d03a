"""The loop and multi-slot paths of the dense-block, histogram and expectation kernels on an MI355X, every amplitude, bin
or value against a host reference on RANDOM states.  Each kernel here has a workgroup cap or a per-pass slot limit; the
code behind it runs only above the sizes (2^20 amplitudes, ~130 terms) at which the other modules compare everything
with numpy, and the full-size tier (28 to 33 qubits) reaches it on structured states or sampled runs only.  The sizes
are the smallest at which each path takes three to four steps (a first, a middle and a last one); every docstring
states the arithmetic and the constants that put its size on the path: whoever changes one moves the size with it.
Each test prints the largest error it reached before it asserts."""
import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.kernel.device import DeviceChunk, plan_expectation
from quantum_simulations_amd.observable import pauli_terms_np
from tests import dynamic_oracle
from tests.pauli_reference import pauli_terms_operator
from tests.test_gpu_kernels import ATOL_KERNEL, _rand_state, _rand_unitary

pytestmark = pytest.mark.gpu


# ---- 1. dense blocks: the loop of a wave over column groups ------------------------------------------------------------
# (k, chunk qubits, the block's qubits in the caller's order)
_DENSE_CASES = [
    (5, 22, [3, 0, 4, 1, 2]),               # the k lowest bits, line bits 0..2 among them
    (5, 22, [19, 21, 17, 20, 18]),          # the k highest bits
    (5, 22, [1, 14, 0, 21, 8]),             # pos[0], pos[1] inside the line, the rest spread out
    (5, 22, [11, 3, 20, 7, 16]),            # mixed, min >= 3
    (6, 23, [2, 5, 0, 3, 1, 4]),
    (6, 23, [20, 17, 22, 19, 18, 21]),
    (6, 23, [2, 9, 0, 22, 15, 5]),
    (6, 23, [12, 3, 22, 8, 17, 5]),
]


def _check_dense(chunk, psi0, qs, M):
    want = psi0.copy()
    orc.apply_kq(want, qs, M)
    chunk.upload(psi0)
    chunk.apply_fused_k(qs, M)
    got = chunk.download()
    err = float(np.max(np.abs(got - want)))
    moved = float(np.max(np.abs(got - psi0)))
    norm2 = chunk.norm2()
    print(f"dense k={len(qs)} n={chunk.k} qubits={qs}: max|got - want| = {err:.3e} (tolerance {ATOL_KERNEL:g}), "
          f"max|after - before| = {moved:.3e}, |norm2 - 1| = {abs(norm2 - 1):.3e}")
    assert err <= ATOL_KERNEL, (qs, err, int(np.argmax(np.abs(got - want))))
    assert moved > 1e-9, (qs, moved)
    assert abs(norm2 - 1.0) < 1e-11, (qs, norm2)


@pytest.mark.parametrize("k,n,qs", _DENSE_CASES, ids=[f"k{k}-" + "_".join(map(str, qs)) for k, _, qs in _DENSE_CASES])
def test_dense_block_where_a_wave_walks_several_column_groups(k, n, qs):
    """k_dense_mfma2<5> / <6>, every amplitude against oracle.dense_oracle.apply_kq, at the smallest chunk where a wave
    takes FOUR column groups: the loop body after the first group -- cb_next, run_stride, the hand-over x = xn, the
    unconditional read-ahead PF == 2 of k = 6 (a wave's last group asks for itself again) -- and the per-XCD region,
    region_base and rot arithmetic over more than one step.  The grid rules of apply_dense_block: col_blocks =
    2^(n - k - 4) column groups of 16 columns; k = 5: min(col_blocks / 4 rounded up to octets, 2 x CUs) workgroups of
    4 waves; k = 6: min(col_blocks / 8 ..., CUs) workgroups of 8 waves.  n = 22, k = 5: 2^13 groups over at most
    512 x 4 = 2^11 waves; n = 23, k = 6: 2^13 groups over at most 256 x 8 = 2^11 waves -- four groups per wave on 256
    CUs (more on fewer), and col_blocks and the grid are multiples of 8, so the region split is active.  Below
    n = 21 (k = 5) / 22 (k = 6) every wave gets exactly one group, which is all the smaller tests enter for these two
    instantiations (the matrix image in LDS, PF == 2).  For k = 3, 4 they do enter the loop -- a wave takes a run of
    four consecutive groups (consec_log2 = 2) -- so `more = false` fails test_dense_k_qubit_block_against_the_oracle
    too (at n = 11, k = 3); what that never takes is the jump cb + 1 + run_stride, which here (consec_log2 = 0) is
    every step.
    Out of reach: the run-to-run jump (run_stride with consec_log2 = 2) of k <= 4 needs more column groups than
    4 x 4 x the grid cap of 2^20 workgroups, i.e. n >= 32; not tested here."""
    psi0 = _rand_state(n, 2200 + 10 * k + qs[0])
    M = _rand_unitary(1 << k, 31 * k + qs[1])
    chunk = DeviceChunk.empty(n)
    try:
        _check_dense(chunk, psi0, qs, M)
    finally:
        chunk.close()


def test_dense_block_column_group_loop_in_the_streaming_form():
    """The same loop in the non-temporal instantiation (k_dense_mfma2<5, NT = true>): a 2^22 view inside a 2^25 parent
    (512 MiB, more than the 256 MiB Infinity Cache: apply_dense_block takes `nt` from the allocation's span) with
    min(qubits) >= 3 (kLaneCut).  The grid is that of the stand-alone 22-qubit chunk: four column groups per wave."""
    n, qs = 22, [10, 3, 21, 6, 15]
    psi0 = _rand_state(n, 2299)
    M = _rand_unitary(32, 99)
    parent = DeviceChunk.empty(25)
    view = parent.view(5 << n, n)
    try:
        view.profile_begin()
        _check_dense(view, psi0, qs, M)
        entry = [e for e in view.profile_end() if e["kernel"].startswith("k_dense")]
        assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["streaming_launches"] == 1, entry
    finally:
        view.close()
        parent.close()


# ---- 2. qsim_probabilities: the walk over loop bits ----------------------------------------------------------------------
def _probabilities_longdouble(p, qs):
    """Bins of the long-double weights p (2^n of them): entry m = the sum over the indices whose bit qs[j] is bit j of m."""
    n = p.size.bit_length() - 1
    drop = tuple(n - 1 - q for q in range(n) if q not in qs)
    kept = sorted(qs, reverse=True)                       # the axes left, in order
    bins = p.reshape([2] * n).sum(axis=drop, dtype=np.longdouble)
    return bins.transpose([kept.index(q) for q in reversed(qs)]).reshape(-1)   # the first axis = the highest bin bit


def _check_probabilities(chunk, psi, selections):
    p = psi.real.astype(np.longdouble) ** 2 + psi.imag.astype(np.longdouble) ** 2
    total = p.sum(dtype=np.longdouble)
    worst_bin = worst_sum = 0.0
    for qs in selections:
        want_ld = _probabilities_longdouble(p, qs)
        want = want_ld.astype(np.float64)
        got = chunk.probabilities(qs)
        rel = float(np.max(np.abs((got - want_ld) / want_ld)))
        rel_sum = float(abs((got.astype(np.longdouble).sum() - total) / total))
        worst_bin, worst_sum = max(worst_bin, rel), max(worst_sum, rel_sum)
        print(f"probabilities n={chunk.k} qubits={qs}: max rel. bin error {rel:.3e}, rel. error of the sum {rel_sum:.3e} (tolerances 1e-12)")
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * want.max(), err_msg=f"n={chunk.k} qubits={qs}")
        assert rel_sum <= 1e-12, (qs, rel_sum)
        again = chunk.probabilities(qs)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), qs
    print(f"probabilities n={chunk.k}: worst rel. bin error {worst_bin:.3e}, worst rel. error of the sum {worst_sum:.3e}")


def test_longdouble_bins_are_in_the_order_of_the_numpy_oracle():
    """(the reference of the two tests below, pinned: same bins as tests.dynamic_oracle.probabilities, unsorted qubits included)"""
    psi = _rand_state(12, 12)
    p = psi.real.astype(np.longdouble) ** 2 + psi.imag.astype(np.longdouble) ** 2
    for qs in ([0], [11], [7, 2, 9], [11, 0, 5, 3, 8, 1, 10, 6]):
        np.testing.assert_allclose(_probabilities_longdouble(p, qs).astype(np.float64), dynamic_oracle.probabilities(psi, qs), rtol=1e-13, atol=0)


def test_probabilities_where_a_workgroup_walks_four_loop_steps():
    """k_hist, every bin against a long-double sum, on a 24-qubit random state: index bits 0..7 are threads, 3 are item
    bits and kHistWgBits = 11 are workgroup bits (qsim_probabilities), so from n = 8 + 3 + 11 + 1 = 23 on the rest are
    LOOP bits, walked by t = ((t | ~loop_mask) + 1) & loop_mask with several steps added into one acc[it].  n = 24: two
    loop bits, four steps.  Which bits they are follows the selection (selected bits above bit 7 become item and
    workgroup bits first; of the free ones the lowest become item bits, the highest workgroup bits):
    nothing selected above bit 7 -> loop bits 11, 12; bits 11 and 12 selected -> the loop moves to 9, 10;
    [9, 11, .., 23] -> item 9, 11, 13, the loop on the NON-ADJACENT bits 8 and 10 (a mask with a hole: what the subset
    enumeration is for).  Below 23 qubits the loop body runs once, which is all the 3-to-20-qubit test enters; the
    30-qubit test walks it on a product state only."""
    n = 24
    selections = [
        [0], [5], [11], [23],                             # r = 1: loop 11, 12 (twice); 9, 10; 11, 12
        [1, 4, 7],                                        # nothing above bit 7: loop bits 11 and 12
        [12, 2, 11],                                      # exactly the would-be loop bits (unsorted): the loop moves to 9, 10
        [23, 0, 9],                                       # unsorted, sub-line + high
        [0, 1, 2, 3, 4, 5, 6, 7],                         # every thread bit: no butterfly at all; loop 11, 12
        [9, 11, 13, 15, 17, 19, 21, 23],                  # loop bits 8 and 10: a mask with a hole
        [16, 0, 23, 5, 12, 2, 7, 10],                     # sub-line and lane bits with high ones, unsorted; loop 11, 13
    ]
    psi = _rand_state(n, 2400)
    chunk = DeviceChunk.from_numpy(psi)
    try:
        _check_probabilities(chunk, psi, selections)
    finally:
        chunk.close()


def test_probabilities_loop_bit_in_the_streaming_form():
    """k_hist<3, NT = true> with one loop bit (two steps): a 23-qubit view (8 thread + 3 item + kHistWgBits = 11 workgroup
    bits + 1) inside a 2^25 parent, 512 MiB > the 256 MiB Infinity Cache."""
    n = 23
    selections = [
        [3],                                              # loop bit 11
        [11],                                             # the would-be loop bit selected: the loop moves to 10
        [22, 1, 10],                                      # unsorted; loop bit 12
        [8, 10, 12, 14, 16, 18, 20, 22],                  # item 8, 10, 12; the free workgroup bits from the top: loop bit 9
        [6, 21, 0, 13, 4, 9, 17, 2],                      # sub-line and lane bits with high ones, unsorted
    ]
    psi = _rand_state(n, 2300)
    parent = DeviceChunk.empty(25)
    view = parent.view(3 << n, n)
    try:
        view.upload(psi)
        view.profile_begin()
        view.probabilities(selections[0])
        entry = [e for e in view.profile_end() if e["kernel"].startswith("k_hist")]
        assert len(entry) == 1 and entry[0]["launches"] == 1 and entry[0]["streaming_launches"] == 1, entry
        _check_probabilities(view, psi, selections)
    finally:
        view.close()
        parent.close()


# ---- 3. qsim_expectation_pauli: the tile loop ---------------------------------------------------------------------------
def _masks(strings):
    """[{qubit: letter}] -> (x, z) masks"""
    xs, zs = [], []
    for ops in strings:
        xs.append(sum(1 << q for q, p in ops.items() if p in "XY"))
        zs.append(sum(1 << q for q, p in ops.items() if p in "ZY"))
    return np.array(xs, dtype=np.uint64), np.array(zs, dtype=np.uint64)


_TILE_N = 22
_TILE_STRINGS = [
    # pass 0: the first X/Y terms fill the tile with bits 0..10, so its outer bits are 11..21 and the two tiles of a
    # workgroup (o and o + 1024) differ in physical bit 21
    {3: "X", 4: "Y", 6: "X", 7: "X", 8: "Y", 9: "X", 10: "X"},
    {0: "Y", 5: "X", 21: "Z", 11: "Z"},
    {},                                                            # the identity
    {21: "Z"},                                                     # Z-only, wholly outside: flips between a workgroup's tiles
    {21: "Z", 15: "Z", 11: "Z"},
    {0: "Z", 2: "Z", 12: "Z", 21: "Z"},                            # low + high
    {q: "Z" for q in range(22)},
    {11: "Z", 10: "Z"},                                            # half inside, flips between neighbouring workgroups
    {1: "Z", 9: "Z"},                                              # wholly inside
    # pass 1: X/Y on high bits pull them into the tile (0..2, 12, 13, 17, 19, 20, 21 + the lowest free 3, 4): the outer
    # bits become LOW ones, the highest of them 18
    {21: "X", 20: "X"},
    {19: "Y"},
    {21: "X", 17: "Y", 18: "Z", 11: "Z", 3: "Z", 0: "Z"},
    {12: "Y", 21: "Z", 18: "Z"},
    {13: "X", 0: "Y", 20: "Z", 5: "Z", 1: "Z"},
    # pass 2
    {14: "X", 15: "Y", 16: "X", 18: "Y", 21: "Z", 6: "Z"},
    {18: "X", 5: "X", 11: "Y", 14: "Z", 2: "Z"},
    # wide: popcount(x | 0b111) = 22 and 17 > kExpTileBits = 11
    {q: "X" for q in range(22)},
    {**{q: "Y" for q in range(8, 22)}, **{q: "Z" for q in range(8)}},
]


@pytest.fixture(scope="module")
def tile_case():
    psi = _rand_state(_TILE_N, 2222)
    x, z = _masks(_TILE_STRINGS)
    want = pauli_terms_operator(psi, x, z)
    want.setflags(write=False)
    psi.setflags(write=False)
    return psi, x, z, want


def _check_tile_loop(chunk, case, what):
    psi, x, z, want = case
    pass_of, tiles = plan_expectation(_TILE_N, x)
    n_wide = int(np.sum(tiles == 0))
    assert n_wide == 2 and len(tiles) - n_wide >= 2, tiles
    assert int(tiles[0]) == (1 << 11) - 1 and int(tiles[1]) >> 12                 # low bits / high bits pulled in
    assert list(pass_of[2:9]) == [0] * 7                                          # the Z-only terms ride in pass 0
    assert all(bin(int(xi) | 0b111).count("1") > 11 for xi in x[-2:])
    got = chunk.expectation_pauli(x, z)
    err = np.abs(got - want)
    print(f"expectation {what} n={_TILE_N}: max|got - want| = {float(err.max()):.3e} at term {int(err.argmax())} (tolerance 1e-12); "
          f"largest |value| {float(np.abs(want).max()):.3e}")
    assert float(err.max()) < 1e-12, (err, int(err.argmax()))
    assert chunk.last_expectation_passes == len(tiles)
    again = chunk.expectation_pauli(x, z)
    assert got.tobytes() == again.tobytes()


def test_expectation_where_a_workgroup_walks_two_tiles(tile_case):
    """k_expect_tile's loop `for (o = blockIdx.x; o < n_tiles; o += gridDim.x)` and k_expect_wide's stride loop on a
    22-qubit random state, against the operator reference (tests/pauli_reference.py).  Tiles hold 2^kExpTileBits = 2^11
    amplitudes and a launch has at most kExpMaxWg = 1024 workgroups, so from n = 11 + 10 + 1 = 22 on a workgroup walks
    more than one tile: here 2^11 tiles, two per workgroup, with the outer sign popc(base & zo) changing between them
    inside one running sum; k_expect_wide (2^21 pairs / 256 threads = 2^13 > 1024 workgroups) takes eight steps.  Up
    to 20 qubits (the every-value test) each workgroup sees one tile; the 30-qubit test walks the loop on GHZ and
    product states only."""
    psi = tile_case[0]
    assert abs(tile_case[3][2] - 1.0) < 1e-12                     # (the identity: the state is normalised)
    chunk = DeviceChunk.from_numpy(psi)
    try:
        _check_tile_loop(chunk, tile_case, "stand-alone")
    finally:
        chunk.close()


def test_expectation_tile_loop_in_the_streaming_form(tile_case):
    """The same passes as k_expect_tile<NT = true> / k_expect_wide<true>: a 2^22 view of a 2^25 parent (512 MiB > the
    256 MiB Infinity Cache); kExpMaxWg = 1024 workgroups over 2^11 tiles as above."""
    parent = DeviceChunk.empty(25)
    view = parent.view(6 << _TILE_N, _TILE_N)
    try:
        view.upload(tile_case[0])
        _check_tile_loop(view, tile_case, "view")
    finally:
        view.close()
        parent.close()


# ---- 4. qsim_expectation_pauli: more than 256 and more than 1024 terms per call ------------------------------------------
_SLOT_N = 13
_SLOT_TILE = 0b1111110110111            # 11 tile bits, the line bits among them; bits 3 and 6 stay outside: four tiles
_SLOT_DUP_XY = (0b1010010010001, 0b0010010001011)       # an X/Y string inside the tile with Z on the outer bit 3
_SLOT_DUP_Z = (0, 0b1000001001100)                      # Z-only, on both outer bits
_SLOT_DUP_XY_AT = (5, 256, 300, 1000)                   # slot rows 0, 1, 1, 3 of a one-pass call (row = position // 256)
_SLOT_DUP_Z_AT = (7, 900)                               # rows 0 and 3


def _slot_terms(count, seed):
    """`count` random strings whose X support lies inside _SLOT_TILE (about 70 % X/Y strings with Z anywhere, the rest
    Z-only, the identity among them)"""
    rng = np.random.default_rng(seed)
    tile_bits = [b for b in range(_SLOT_N) if (_SLOT_TILE >> b) & 1]
    xs, zs = [], []
    for t in range(count):
        x = 0
        if rng.random() < 0.7:
            for b in rng.choice(tile_bits, size=int(rng.integers(1, 7)), replace=False):
                x |= 1 << int(b)
        z = int(rng.integers(0 if x else 1, 1 << _SLOT_N))
        xs.append(x)
        zs.append(z)
    xs[3], zs[3] = 0, 0
    return xs, zs


@pytest.fixture(scope="module")
def slot_case():
    """2100 terms and their values; the shorter calls are prefixes of this list (one reference, shared)"""
    psi = _rand_state(_SLOT_N, 1313)
    xs, zs = _slot_terms(2100, 13)
    for at in _SLOT_DUP_XY_AT:
        xs[at], zs[at] = _SLOT_DUP_XY
    for at in _SLOT_DUP_Z_AT:
        xs[at], zs[at] = _SLOT_DUP_Z
    x, z = np.array(xs, dtype=np.uint64), np.array(zs, dtype=np.uint64)
    want = pauli_terms_np(psi, x, z)
    for a in (psi, x, z, want):
        a.setflags(write=False)
    return psi, x, z, want


@pytest.mark.parametrize("count", [257, 600, 1024, 1025, 2100])
def test_expectation_with_more_terms_than_one_slot_row(slot_case, count):
    """k_expect_tile's slot rows s >= 1 and the split of a pass at kExpMaxTerms = 1024, every value against
    pauli_terms_np on a 13-qubit state (four tiles; the path does not depend on n).  A workgroup has kBlock = 256
    threads; a pass of more than 256 terms runs with slices == 1, thread tid evaluating the terms tid + 256 s of slot
    rows s = 0 .. kExpSlots - 1 = 3 (t = tid / slices + per * s) and handing them over through red[s * kBlock + tid].
    Every X support lies inside one set of 11 tile bits, so the planner keeps the terms in one pass by width and
    splits by count alone: 257 and 600 terms -> one pass (rows 0..1 and 0..2), 1024 -> one pass of exactly 1024 (row
    3 full), 1025 and 2100 -> a full pass and what follows.  The largest list any other GPU test sends has ~130 terms.
    One (x, z) pair sits at several positions of a pass, in slot rows 0 and 3 among them: with one `slices` value
    per pass the summation order is the same, so its values are bitwise equal."""
    psi, x, z, want = slot_case
    x, z, want = x[:count], z[:count], want[:count]
    pass_of, tiles = plan_expectation(_SLOT_N, x)
    counts = list(np.bincount(pass_of))
    assert int(tiles[0]) == _SLOT_TILE and 0 not in [int(t) for t in tiles]
    if count <= 1024:
        assert counts == [count] and count > 256
    else:
        assert counts[0] == 1024 and len(counts) >= 2 and sum(counts) == count and all(c <= 1024 for c in counts)
    chunk = DeviceChunk.from_numpy(psi)
    try:
        got = chunk.expectation_pauli(x, z)
        err = np.abs(got - want)
        print(f"expectation {count} terms, passes {counts}: max|got - want| = {float(err.max()):.3e} at term {int(err.argmax())} (tolerance 1e-12)")
        assert float(err.max()) < 1e-12, (count, float(err.max()), int(err.argmax()))
        assert chunk.last_expectation_passes == len(tiles)
        assert got.tobytes() == chunk.expectation_pauli(x, z).tobytes()
        if count <= 1024:                                      # one pass: a term's table position is its position in the call
            for at in (_SLOT_DUP_XY_AT, _SLOT_DUP_Z_AT):
                at = [a for a in at if a < count]
                assert len({got[a].tobytes() for a in at}) == 1, (at, got[at])
            assert [a // 256 for a in _SLOT_DUP_XY_AT if a < count][:2] == [0, 1]        # (257 terms: row 1 holds this one alone)
        if count == 1024:
            assert [a // 256 for a in _SLOT_DUP_XY_AT] == [0, 1, 1, 3] and [a // 256 for a in _SLOT_DUP_Z_AT] == [0, 3]
        # about 20 of the terms in a call of their own (slices = 8 > 1: another deal of threads, another summation order)
        pick = np.unique(np.concatenate([np.linspace(0, count - 1, 18).astype(int), [5, 256]]))
        assert 18 <= len(pick) <= 20 and 4 * 2 * len(pick) <= 256 < 8 * 2 * len(pick)      # the launcher's rule for slices = 8
        sub = chunk.expectation_pauli(x[pick], z[pick])
        sub_err = float(np.max(np.abs(sub - got[pick])))
        print(f"expectation {count} terms: max|subset call - big call| = {sub_err:.3e} (tolerance 1e-12)")
        assert sub_err < 1e-12, (count, sub_err)
    finally:
        chunk.close()


def test_expectation_passes_split_by_width_and_by_count(slot_case):
    """One list whose passes split BOTH ways: 1100 X/Y strings inside one 11-bit tile (a pass of kExpMaxTerms = 1024 and
    the rest), 30 strings with X on the two bits that tile leaves out (another tile by width), two strings wider than
    kExpTileBits = 11 bits (a k_expect_wide pass each) and Z-only strings that fill what room there is."""
    psi, x_all, z_all, _ = slot_case
    rng = np.random.default_rng(131)
    keep = np.flatnonzero(x_all)[:1100]
    xs, zs = [int(v) for v in x_all[keep]], [int(v) for v in z_all[keep]]
    other = [0b1001000, 0b1001000 | 1 << 12, 0b1000000 | 1 << 4, 0b0001000 | 1 << 9 | 1]      # X on bits 3 and / or 6
    for j in range(30):
        xs.append(other[j % len(other)])
        zs.append(int(rng.integers(0, 1 << _SLOT_N)))
    full = (1 << _SLOT_N) - 1
    xs += [full, full & ~1]
    zs += [0b1010101010101, full]
    for _ in range(100):
        xs.append(0)
        zs.append(int(rng.integers(1, 1 << _SLOT_N)))
    # the first 300 stay in front (they complete pass 0's tile before a string of another tile can claim a bit of it:
    # the planner is first-fit); everything behind them is shuffled
    order = np.concatenate([np.arange(300), 300 + rng.permutation(len(xs) - 300)])
    x, z = np.array(xs, dtype=np.uint64)[order], np.array(zs, dtype=np.uint64)[order]
    pass_of, tiles = plan_expectation(_SLOT_N, x)
    counts = list(np.bincount(pass_of))
    tile_masks = [int(t) for t in tiles if t]
    assert counts[0] == 1024 and tile_masks[0] == _SLOT_TILE     # split by count: 1100 X/Y strings fit this tile, 76 had to go on
    assert len(set(tile_masks)) >= 2 and len(tiles) - len(tile_masks) == 2, (counts, tiles)   # split by width; both wide passes
    want = pauli_terms_np(psi, x, z)
    chunk = DeviceChunk.from_numpy(psi)
    try:
        got = chunk.expectation_pauli(x, z)
        err = np.abs(got - want)
        print(f"expectation mixed list, passes {counts}: max|got - want| = {float(err.max()):.3e} at term {int(err.argmax())} (tolerance 1e-12)")
        assert float(err.max()) < 1e-12, (float(err.max()), int(err.argmax()))
        assert chunk.last_expectation_passes == len(tiles)
        assert got.tobytes() == chunk.expectation_pauli(x, z).tobytes()
    finally:
        chunk.close()
