"""Unit-diagonal butterflies for real 2x2 gates (OPC_UNIT1), on the CPU: which records the lowering rewrites
(csrc/tile_groups.h lower_unit_real, reached through `planner.lower_images`), their form, sign and ratios, where the
factors of a pass go, and that a lowered plan is still the oracle's program.

Planned images (`planner.plan_ops`) keep real 2x2 records as OPC_REAL1; the rewrite happens where `qsim_apply_ops*` hand
an image to the device.  `raise_images` below undoes it record by record in numpy -- OPC_UNIT1 (p, q, form, sign) back to
the OPC_REAL1 record of the UNSCALED butterfly, the factor staying where the lowering put it -- so that
tests/tile_interpreter.py walks exactly what the device would run.  Needs the built library, no GPU."""
import functools

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.runner import engine, engine_cost
from tests import engine_cases as ec
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import _rand_state, _random_ops
from tests.test_pass_search_cpu import _bench_ops

UNIT1 = 118                        # QS_ENT_UNIT1 (csrc/gen_tile_engine.py): + 4 * target register + 2 * (form A) + (sigma = -1)
GROUPS = (ti.OPC["GROUP"], ti.OPC["GROUP_FIRST"], ti.OPC["GROUP_DIRECT"])
ENDS = (ti.OPC["END"], ti.OPC["END_DIRECT"])
PREDS = (ti.OPC["PRED_OUTER"], ti.OPC["PRED_LANE"], ti.OPC["PRED_OUTER_ZERO"])
X = np.array([[0, 1], [1, 0]], dtype=complex)
Z = np.diag([1, -1]).astype(complex)
H = orc.gate_matrix("H")
ANGLES = [0.0, 1e-9, np.pi / 2 - 1e-9, np.pi / 2, np.pi / 2 + 1e-9, np.pi, 3 * np.pi / 2, 2 * np.pi - 1e-9] + \
    [float(t) for t in np.random.default_rng(2024).uniform(0, 2 * np.pi, 20)]


def ry(theta):
    return orc.gate_matrix("RY", {"theta": theta})


def family(theta):
    """RY and what the rewrite makes of it with an X or a Z on either side"""
    R = ry(theta)
    return {"RY": R, "RY.X": R @ X, "X.RY": X @ R, "RY.Z": R @ Z, "Z.RY": Z @ R}


def gate_records(img):
    """[(byte offset, entry, case, predicated, next)] of the gate records of an image, lowered or not"""
    raw = img.tobytes()
    out, off = [], planner.STREAM_OFF
    while True:
        d = np.frombuffer(raw, dtype="<u4", count=4, offset=off)
        entry, nxt = int(d[0]) // 4, int(d[1])
        if entry in ENDS:
            return out
        if entry not in GROUPS:
            out.append((off, entry, (int(d[3]) >> 16) // 4, entry in PREDS, nxt))
        off = nxt


def doubles(img, off, count):
    return np.frombuffer(img.tobytes(), dtype="<f8", count=count, offset=off + 16)


def unit_records(img):
    """[(target register, form A, sigma, p, q, s)] of the OPC_UNIT1 records of a lowered image"""
    out = []
    for off, entry, case, pred, _ in gate_records(img):
        if UNIT1 <= case < UNIT1 + 12:
            assert entry == case and not pred, "OPC_UNIT1 is never predicated"
            v = case - UNIT1
            p, q, s, pad = doubles(img, off, 4)
            assert pad == 0.0
            out.append((v // 4, bool(v & 2), -1.0 if v & 1 else 1.0, float(p), float(q), float(s)))
    return out


def butterfly(form_a, sigma, p, q):
    return np.array([[p, 1.0], [sigma, q]]) if form_a else np.array([[1.0, p], [q, sigma]])


def raise_images(lowered):
    """Lowered images with every OPC_UNIT1 record written back as the OPC_REAL1 record of its unscaled butterfly."""
    out = lowered.copy()
    flat = out.view(np.uint8).reshape(len(out), planner.IMAGE_BYTES)
    for i, img in enumerate(lowered):
        for off, entry, case, _, _ in gate_records(img):
            if UNIT1 <= case < UNIT1 + 12:
                v = case - UNIT1
                p, q = doubles(img, off, 2)
                m = butterfly(bool(v & 2), -1.0 if v & 1 else 1.0, p, q).reshape(4)
                real1 = 4 * (ti.OPC["REAL1"] + v // 4)
                flat[i, off:off + 4] = np.frombuffer(np.uint32(real1).tobytes(), dtype=np.uint8)
                flat[i, off + 12:off + 16] = np.frombuffer(np.uint32(real1 << 16).tobytes(), dtype=np.uint8)
                flat[i, off + 16:off + 48] = np.frombuffer(m.astype("<f8").tobytes(), dtype=np.uint8)
    return out


def qualifies(M) -> bool:
    """numpy statement of the family: a real 2x2 record (not anti-diagonal, not a phase gate or the identity) with
    |m0| == |m3| and |m1| == |m2| that is not the Hadamard shape"""
    if np.any(M.imag != 0):
        return False
    m = M.real.reshape(4)
    if (m[0] == 0 and m[3] == 0) or (m[1] == 0 and m[2] == 0 and m[0] == 1):
        return False
    if m[0] == m[1] == m[2] == -m[3]:
        return False
    return bool(abs(m[0]) == abs(m[3]) and abs(m[1]) == abs(m[2]))


def lowered_cases(n, ops):
    images = planner.plan_ops(n, ops)
    low, count = planner.lower_images(images)
    assert count == sum(len(unit_records(img)) for img in low)
    return images, low


def cases_of(images):
    return [case for img in images for _, _, case, _, _ in gate_records(img)]


def ulp_close(a, b, ulps=2):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


# ---------------------------------------------------------------------------------------------------------------------
def test_which_records_become_unit1():
    """With a complex 2x2 in the pass to take the factor: RY and its products with X and Z at every angle of the list;
    H stays OPC_HAD1; a controlled RY (register control), one under a lane and one under an outer predicate, and a
    real matrix outside the family stay OPC_REAL1."""
    n, host = 14, ([8], ec.M_DENSE)
    for theta in ANGLES:
        for name, M in family(theta).items():
            if M[0, 0] == 0 and M[1, 1] == 0:
                continue                   # (anti-diagonal: OPC_ANTI1 / OPC_SWAP1, never a real 2x2 record)
            if M[0, 1] == 0 and M[1, 0] == 0 and M[0, 0] == 1:
                continue                   # (the identity or a phase gate)
            _, low = lowered_cases(n, [host, ([9], M)])
            units = unit_records(low[0])
            assert len(units) == 1 and units[0][0] == 1, (name, theta, cases_of(low))
    R = ry(0.7)
    images, low = lowered_cases(n, [host, ([9], H)])
    assert ti.OPC["HAD1"] + 1 in cases_of(low) and not unit_records(low[0])
    for what, ops in (("register control", [host, ec.controlled(10, 9, R, True)]),
                      ("lane predicate", [host, ec.controlled(4, 9, R, True)]),
                      ("outer predicate", [host, ec.controlled(12, 9, R, True)]),
                      ("outside the family", [host, ([9], np.diag([1, 0.5]) @ R)])):
        images, low = lowered_cases(n, ops)
        assert not unit_records(low[0]), what
        assert any(ti.OPC["REAL1"] <= c < ti.OPC["REAL1"] + 9 for c in cases_of(low)), what
        assert low.tobytes() == images.tobytes(), what


def test_form_sign_and_ratios():
    """Form D exactly when |m0| >= |m1| (the tie at theta = pi / 2 included), |p|, |q| <= 1, sigma = +-1, and the 2x2
    rebuilt from (s, p, q, sigma, form) is the input to 2 ulp."""
    n, host = 11, ([8], ec.M_DENSE)
    seen = set()
    for theta in ANGLES:
        for name, M in family(theta).items():
            m = M.real
            if (m[0, 0] == 0 and m[1, 1] == 0) or (m[0, 1] == 0 and m[1, 0] == 0 and m[0, 0] == 1):
                continue
            _, low = lowered_cases(n, [host, ([10], M)])
            (J, form_a, sigma, p, q, s), = unit_records(low[0])
            assert J == 2
            assert form_a == (not abs(m[0, 0]) >= abs(m[0, 1])), (name, theta)
            assert abs(p) <= 1 and abs(q) <= 1 and s == (m[0, 1] if form_a else m[0, 0])
            assert ulp_close(s * butterfly(form_a, sigma, p, q), m), (name, theta)
            seen.add((form_a, sigma))
    assert seen == {(False, 1.0), (False, -1.0), (True, 1.0), (True, -1.0)}
    c = np.sqrt(0.5)                   # an exact tie |m0| == |m1| (RY(pi / 2) itself may miss it by an ulp): form D
    for tie in (np.array([[c, -c], [c, c]]), np.array([[c, c], [-c, c]]), np.array([[-c, c], [c, c]])):
        _, low = lowered_cases(n, [host, ([10], tie.astype(complex))])
        (J, form_a, sigma, p, q, s), = unit_records(low[0])
        assert form_a is False and s == tie[0, 0] and abs(p) == 1 and abs(q) == 1
        assert np.array_equal(s * butterfly(form_a, sigma, p, q), tie)


def _six_and_two_h(with_host):
    thetas = [0.3, 1.1, 2.0, 2.9, 4.2, 5.5]
    mats = [ry(thetas[0]), ry(thetas[1]) @ X, Z @ ry(thetas[2]), ry(thetas[3]), X @ ry(thetas[4]), ry(thetas[5]) @ Z]
    ops = [([3 + i], M) for i, M in enumerate(mats)] + [([9], H), ([10], 0.6 * np.sqrt(2) * H)]
    if with_host:
        ops.insert(4, ([0], ec.M_DENSE))
    return ops, mats


def test_the_factors_of_a_pass():
    """6 gates of the family and 2 H in one pass: the product of their factors lands in the unconditional complex 2x2 of
    the pass when there is one; else the last of the six stays OPC_REAL1 and carries it (no OPC_SCALE record: the planner
    had folded the Hadamard factors into a real 2x2 already)."""
    for with_host in (True, False):
        ops, mats = _six_and_two_h(with_host)
        images, low = lowered_cases(11, ops)
        assert len(low) == 1
        units = unit_records(low[0])
        assert len(units) == (6 if with_host else 5)
        # (the planner folds the Hadamard factors into the FIRST unconditional 2x2 of the pass, which may be one of the six:
        # its s then carries them)
        product = float(np.prod([u[5] for u in units]))
        had = H[0, 0].real * (0.6 * np.sqrt(2) * H)[0, 0].real
        own = float(np.prod([M.real[0, 1] if abs(M.real[0, 1]) > abs(M.real[0, 0]) else M.real[0, 0] for M in mats]))
        recs = gate_records(low[0])
        scale = [r for r in recs if r[2] == ti.OPC["SCALE"]]
        if with_host:
            assert not scale
            (off, _, case, _, nxt), = [r for r in recs if ti.OPC["DENSE1"] <= r[2] < ti.OPC["DENSE1"] + 3]
            got = np.concatenate([doubles(low[0], off, 6), doubles(low[0], nxt - 32, 2)])
            want = np.stack([ec.M_DENSE.real.reshape(4), ec.M_DENSE.imag.reshape(4)], axis=1).reshape(8) * product
            assert ulp_close(got, want, 2)
            assert abs(product - had * own) <= 8 * np.spacing(abs(product))
        else:
            assert not scale
            (off, _, case, _, _), = [r for r in recs if ti.OPC["REAL1"] <= r[2] < ti.OPC["REAL1"] + 3]
            kept = doubles(low[0], off, 4)
            larger = kept[1] if abs(kept[1]) > abs(kept[0]) else kept[0]
            assert abs(larger - had * own) <= 8 * np.spacing(abs(had * own))
            extra = [tuple(np.round(kept / larger, 12))]
        # every 2x2 of the family comes back from its record, up to the factor taken out of it
        rebuilt = sorted([tuple(np.round(butterfly(*u[1:5]).reshape(4), 12)) for u in units] + (extra if not with_host else []))
        assert rebuilt == sorted(tuple(np.round((M.real / (M.real[0, 1] if abs(M.real[0, 1]) > abs(M.real[0, 0]) else M.real[0, 0])).reshape(4), 12))
                                 for M in mats)


def test_a_pass_with_nothing_to_take_the_factor_keeps_one_real_record():
    """No complex / anti-diagonal 2x2, no H: the last gate of the family stays OPC_REAL1 and carries the product (an
    OPC_SCALE record would cost more than the FMA it saves); a single such gate is left alone."""
    images, low = lowered_cases(11, [([8], ry(0.4)), ([9], ry(1.9)), ([10], ry(2.6) @ X)])
    units = unit_records(low[0])
    assert len(units) == 2 and ti.OPC["SCALE"] not in cases_of(low)
    (off, _, case, _, _), = [r for r in gate_records(low[0]) if ti.OPC["REAL1"] <= r[2] < ti.OPC["REAL1"] + 3]
    assert ulp_close(doubles(low[0], off, 4), (ry(2.6) @ X).real.reshape(4) * units[0][5] * units[1][5], 4)
    images, low = lowered_cases(11, [([8], ry(0.4)), ec.phase1(9, ec.P_GENERIC)])
    assert low.tobytes() == images.tobytes()


@pytest.mark.parametrize("n", [9, 11, 12, 13])
def test_lowered_plans_walk_into_the_oracle_state(n):
    """Random lists (RY, H, X, controlled and dense gates among them): the lowered images, walked record by record,
    give the oracle's state; so do the planned ones, and the two walks agree to 1e-14."""
    rewritten = 0
    for seed in range(3):
        ops = _random_ops(n, 90, 50 * n + seed) + [([q], ry(0.3 + q)) for q in range(n)]
        images = planner.plan_ops(n, ops)
        low, count = planner.lower_images(images)
        rewritten += count
        psi0 = _rand_state(n, 900 + n + seed)
        want = psi0.copy()
        orc.apply_ops(want, ops)
        a, b = psi0.copy(), psi0.copy()
        ti.run(a, images)
        ti.run(b, raise_images(low))
        assert float(np.max(np.abs(b - want))) <= 1e-12
        assert float(np.max(np.abs(a - b))) <= 1e-14
    assert rewritten >= 3 * n // 2


@functools.lru_cache(maxsize=None)
def bench_counts(n):
    """(unconditional OPC_REAL1 records, those the lowering takes) of the bench circuit's plan on the identity layout,
    built as `SingleGpuEngine.plan_batches` builds it: rewrite, searched tiles, the priced variant, its placement."""
    costs = engine_cost.table()
    ops = _bench_ops(n)
    plain = planner.rewrite_ops(n, ops)
    masks = planner.search_tiles(n, plain)
    priced = planner.rewrite_ops(n, ops, None, costs)
    kept, placed, _ = engine.priced_variant(n, [plain], [priced], [masks], costs)
    images = planner.plan_ops(n, kept[0], masks, placed[0])
    low, count = planner.lower_images(images)
    real = sum(1 for img in images for _, entry, case, pred, _ in gate_records(img)
               if not pred and ti.OPC["REAL1"] <= case < ti.OPC["REAL1"] + 3)
    return real, count, len(images)


@pytest.mark.parametrize("n", [28, 30])
def test_most_real_records_of_the_bench_plan_qualify(n):
    real, unit, passes = bench_counts(n)
    print(f"{n} qubits: {passes} passes, {real} unconditional OPC_REAL1 records, {unit} lowered to OPC_UNIT1")
    assert unit >= 0.5 * real
