"""The priced planner on the CPU: rule (d) of the op rewrite (csrc/op_rewrite.h, `qsim_rewrite_ops_priced`), the placement
of the ops that need no tile (csrc/tile_search.h `plan_balance`, `qsim_plan_balance`, `qsim_plan_ops_placed`) and the
engine cost table they are handed (runner/engine_cost.py).  Plans are walked by tests/tile_interpreter.py against the
dense oracle; pass counts and modelled times are set against the plan built with the pricing switched off (the table
argument None: the planner as it was).  No device involved."""
import functools

import numpy as np
import pytest

from oracle import dense_oracle as orc
from quantum_simulations_amd import circuits as gen
from quantum_simulations_amd.kernel import planner
from quantum_simulations_amd.runner import engine, engine_cost
from tests import tile_interpreter as ti
from tests.test_gpu_kernels import _rand_state
from tests.test_op_rewrite_cpu import _lists, _same, collapse_factor, device_cases, mixed_ops
from tests.test_pass_search_cpu import _bench_ops

PLAN_TOL = 1e-12                   # interpreter walk of a priced plan against the oracle (the issue's bound)
EQUIV_TOL = 1e-13                  # rule (d): output list against input list on a random state (the issue's bound)
COSTS = engine_cost.table()


def _batch(cd, n):
    from quantum_simulations_amd.circuit.fusion import batch_levels
    from quantum_simulations_amd.circuit.io import levelize, validate_circuit_dict
    batches = [p["local_ops"] for p in batch_levels(levelize(validate_circuit_dict(cd)), n)]
    assert len(batches) == 1
    return batches[0]


def priced_plan(n, ops, costs):
    """(planned list, tiles, placement or None, modelled ms, passes the plan really takes) on the identity layout, as
    `SingleGpuEngine.plan_batches` builds a plan: the tiles searched on the rewritten list; pricing on (costs = the
    table): whichever of the list under rule (d) and the rewritten list, placed, `engine.priced_variant` keeps; off (None):
    the rewritten list first come, priced by the table without any placement."""
    plain = planner.rewrite_ops(n, ops)
    masks = planner.search_tiles(n, plain)
    if costs is None:
        mem = engine.pass_memory_us(n, masks)
        _, before, _ = planner.balance(n, plain, masks, mem, COSTS, place=False)
        ms = round(float(np.maximum(mem, before).sum()) / 1e3, 6)              # (the rounding of `engine.priced_variant`)
        return plain, masks, None, ms, planner.pass_count(n, plain, masks)
    priced = planner.rewrite_ops(n, ops, None, costs)
    kept, placed, split = engine.priced_variant(n, [plain], [priced], [masks], costs)
    return kept[0], masks, placed[0], split["passes"], planner.pass_count(n, kept[0], masks, placed[0])


def _qft_like(n, seed):
    """phase heavy: the QFT's controlled rotations with T / S / Z and a few H and CNOT between them"""
    rng = np.random.default_rng(seed)
    ops = _batch(gen.generate_ghz_qft(n), n)
    extra = []
    for i, op in enumerate(ops):
        extra.append(op)
        if i % 3 == 0:
            extra.append(([int(rng.integers(n))], orc.gate_matrix(("T", "S", "Z")[int(rng.integers(3))])))
    return extra


@functools.lru_cache(maxsize=None)
def _small_lists():
    """(name, n, ops): random 1q+CX, Clifford+T, phase-heavy and the mixed list of the device cases at 12..14 qubits"""
    out = []
    for n in (12, 13, 14):
        out += [(f"{name}{n}", n, ops) for name, _, ops in device_cases(n)]
        out.append((f"qft_like{n}", n, _qft_like(n, 40 + n)))
    return out


def test_priced_plans_walk_into_the_oracle_state():
    """rewrite (d) -> search -> placement -> pass images under the placement: the oracle's state of the ORIGINAL list, in
    exactly the searched passes"""
    moved = 0
    for name, n, ops in _small_lists():
        rewritten, masks, placed, _, passes = priced_plan(n, ops, COSTS)
        images = planner.plan_ops(n, rewritten, masks, placed)
        assert len(images) == passes <= len(masks), name
        moved += 0 if placed is None else int((placed > 0).sum())
        psi = _rand_state(n, 700 + n)
        want = psi.copy()
        orc.apply_ops(want, ops)
        ti.run(psi, images)
        np.testing.assert_allclose(psi, want, rtol=0, atol=PLAN_TOL, err_msg=name)
    print("ops placed later than first come over the lists:", moved)


def test_any_placement_is_a_correct_program():
    """earliest passes drawn at random (not the balance's): an op that is told to wait blocks what depends on it, so the
    amplitudes stay the oracle's whatever the values -- only the pass count may grow.  And a balance under a memory model
    with room in every second pass moves ops (the path the small lists above may not reach)."""
    rng = np.random.default_rng(5)
    balanced = 0
    for name, n, ops in _small_lists()[::2]:
        rewritten = planner.rewrite_ops(n, ops, None, COSTS)
        masks = planner.search_tiles(n, rewritten)
        placements = [rng.integers(0, len(masks) + 1, size=len(rewritten)).astype(np.int32)]
        mem = np.where(np.arange(len(masks)) % 2 == 0, 0.0, 1e9)
        earliest, before, after = planner.balance(n, rewritten, masks, mem, COSTS)
        if earliest.any():                 # (a placement is only made when the model prices it lower, in the same passes)
            assert np.maximum(mem, after).sum() < np.maximum(mem, before).sum(), name
            assert planner.pass_count(n, rewritten, masks, earliest) == len(masks), name
            placements.append(earliest)
            balanced += 1
        else:
            assert np.array_equal(before, after), name
        for place in placements:
            images = planner.plan_ops(n, rewritten, masks, place)
            psi = _rand_state(n, 800 + n)
            want = psi.copy()
            orc.apply_ops(want, ops)
            ti.run(psi, images)
            np.testing.assert_allclose(psi, want, rtol=0, atol=PLAN_TOL, err_msg=name)
    assert balanced >= 3


def _rule_d_lists():
    """the seeded mixed lists (non-unitary collapse factors among them; every third framed by X / Y at both ends), an
    all-diagonal list, and lists with a frame pending at both ends around diagonals and dense gates"""
    out = list(_lists())
    rng = np.random.default_rng(11)
    diag = []
    for _ in range(60):
        if rng.random() < 0.5:
            diag.append(([int(rng.integers(8))], orc.gate_matrix(("Z", "S", "T")[int(rng.integers(3))])))
        else:
            a, b = (int(x) for x in rng.choice(8, size=2, replace=False))
            diag.append(([a, b], orc.gate_matrix(("CZ", "CR")[int(rng.integers(2))], {"k": 3})))
    out.append((8, diag))
    X, Y, H, T, Z, S = (orc.gate_matrix(g) for g in ("X", "Y", "H", "T", "Z", "S"))
    RY = orc.gate_matrix("RY", {"theta": 0.9})
    CNOT, CZ = orc.gate_matrix("CNOT"), orc.gate_matrix("CZ")
    out.append((6, [([0], X), ([1], Y), ([0], T), ([0, 1], CNOT), ([1], Z), ([1], RY), ([0], S), ([0, 2], CZ), ([0], H), ([0], T),
                    ([2], Z), ([2], RY), ([2], T), ([1, 2], CNOT), ([1], S), ([0], collapse_factor(0, 1.2)), ([0], Z), ([0], RY),
                    ([1], Y), ([2], X)]))
    out.append((7, mixed_ops(7, 80, 9100, framed=True)))
    return out


def test_rule_d_gives_the_same_state():
    worst, merged = 0.0, 0
    for case, (n, ops) in enumerate(_rule_d_lists()):
        plain, priced = planner.rewrite_ops(n, ops), planner.rewrite_ops(n, ops, None, COSTS)
        merged += len(plain) - len(priced)
        psi = _rand_state(n, 1900 + case)
        want = psi.copy()
        orc.apply_ops(want, ops)
        orc.apply_ops(psi, priced)
        worst = max(worst, float(np.max(np.abs(psi - want))))
        np.testing.assert_allclose(psi, want, rtol=0, atol=EQUIV_TOL, err_msg=f"case {case}")
    print(f"max |diff| {worst:.2e}; rule (d) removed {merged} ops over {len(_rule_d_lists())} lists")
    assert merged > 0


def test_rule_d_output_is_a_fixed_point_and_needs_no_more_tiles():
    for case, (n, ops) in enumerate(_rule_d_lists()):
        stats, plain_stats = {}, {}
        out = planner.rewrite_ops(n, ops, stats, COSTS)
        planner.rewrite_ops(n, ops, plain_stats)
        assert stats["need_tile_out"] <= stats["need_tile_in"], (case, stats)
        assert stats["need_tile_out"] <= plain_stats["need_tile_out"], (case, stats, plain_stats)    # never more than rules (a)-(c) leave
        assert stats["ops_out"] == len(out) <= plain_stats["ops_out"], case
        again = {}
        assert _same(planner.rewrite_ops(n, out, again, COSTS), out), case
        assert again["need_tile_out"] == again["need_tile_in"] == stats["need_tile_out"], case


def test_rule_d_follows_the_table():
    """Z always pays; S or T into a real 2x2 make a complex one and pay only where the table says so; a table that prices
    the diagonals at nothing merges nothing; no table is the unpriced call"""
    Z, T, H = orc.gate_matrix("Z"), orc.gate_matrix("T"), orc.gate_matrix("H")
    RY = orc.gate_matrix("RY", {"theta": 0.7})
    CZ = orc.gate_matrix("CZ")
    ops = [([0], RY), ([0, 1], CZ), ([0], Z), ([1], RY), ([1], T), ([2], RY), ([1, 2], CZ)]
    out = planner.rewrite_ops(4, ops, None, COSTS)
    c = dict(zip(engine_cost.ENTRIES, COSTS))
    assert c["phase_neg"] > 0                                                # (then RY Z -> one real 2x2 is cheaper)
    kept_t = c["phase"] + c["real1"] <= c["dense1"]
    assert len(out) == len(ops) - 1 - (0 if kept_t else 1), out
    np.testing.assert_allclose(out[0][1], Z @ RY, atol=1e-15)                 # D U: the dense gate came first
    free = COSTS.copy()
    for name in ("phase", "phase_neg", "phase_i"):
        free[engine_cost.ENTRIES.index(name)] = 0.0
    assert _same(planner.rewrite_ops(4, ops, None, free), planner.rewrite_ops(4, ops))
    assert _same(planner.rewrite_ops(4, ops, None, None), planner.rewrite_ops(4, ops))
    with pytest.raises(ValueError):
        planner.rewrite_ops(4, ops, None, COSTS[:5])                          # a short table is an error, not "off"


@functools.lru_cache(maxsize=None)
def _bench_layout(n):
    plain, priced = planner.rewrite_ops(n, _bench_ops(n)), planner.rewrite_ops(n, _bench_ops(n), None, COSTS)
    return engine.choose_plan_layout(n, [plain], engine_costs=COSTS, priced_batches=[priced])


@pytest.mark.parametrize("n, passes", [(28, 13), (30, 15)])
def test_bench_lists_keep_their_pass_counts(n, passes):
    """the depth-40 bench lists under the priced planner, as `SingleGpuEngine.plan` builds them: at most 13 passes at 28
    qubits and 15 at 30 (what the planner reached with the pricing off), the placement included"""
    l2p, masks, info = _bench_layout(n)
    print(n, {k: v for k, v in info.items() if k not in ("placed", "planned")})
    assert info["passes_chosen"] <= passes
    assert planner.pass_count(n, info["planned"][0], masks[0], info["placed"][0]) == info["passes_chosen"]
    split = info["model_split_ms"]
    assert split["rule_d_ops"] > 0 and split["passes"] < split["passes_unpriced"] and split["memory"] <= split["passes"]


def _families(n):
    return [("bench_random_1q_cx_d40", _bench_ops(n)), ("ghz_qft", _batch(gen.generate_ghz_qft(n), n)),
            ("clifford_t_d60", _batch(gen.random_clifford_t_circuit(n, depth=60), n)),
            ("random_1q_cx_d40_seed7", _batch(gen.random_1q_cx_circuit(n, depth=40, seed=7), n))]


@pytest.mark.parametrize("n", [28, 30])
def test_workload_families_no_more_passes_and_no_more_modelled_time(n):
    """the families of profiles/r08_pass_search_cpu.txt on the identity layout: the priced plan has no more passes than the
    plan with the pricing off unless its modelled time is lower (both printed), and its modelled ms are never higher"""
    for name, ops in _families(n):
        _, _, _, ms0, passes0 = priced_plan(n, ops, None)
        kept, _, placed, ms1, passes1 = priced_plan(n, ops, COSTS)
        moved = 0 if placed is None else int((placed > 0).sum())
        print(f"{name} {n}: passes {passes0} -> {passes1} ({len(kept)} ops, {moved} placed later), modelled ms {ms0:.3f} -> {ms1:.3f}")
        assert passes1 <= passes0 or ms1 < ms0, name           # the passes the planned list really takes under its placement
        assert ms1 <= ms0, name


def test_small_lists_no_more_modelled_time():
    for name, n, ops in _small_lists():
        _, _, _, ms0, passes0 = priced_plan(n, ops, None)
        _, _, _, ms1, passes1 = priced_plan(n, ops, COSTS)
        print(f"{name}: passes {passes0} -> {passes1}, modelled ns {1e6 * ms0:.2f} -> {1e6 * ms1:.2f}")
        assert passes1 <= passes0 or ms1 < ms0, name
        assert ms1 <= ms0, name


def test_balance_rejects_bad_input():
    n, ops = 12, device_cases(12)[0][2]
    masks = planner.search_tiles(n, ops)
    with pytest.raises(ValueError):
        planner.balance(n, ops, masks, np.zeros(len(masks) + 1), COSTS)
    with pytest.raises(ValueError):
        planner.balance(n, ops, masks, np.zeros(len(masks)), COSTS[:3])
    with pytest.raises(ValueError):
        planner.plan_ops(n, ops, masks, np.zeros(len(ops) + 1, dtype=np.int32))
    earliest, before, after = planner.balance(n, ops, masks, np.full(len(masks), 1e9), COSTS)      # memory bound everywhere
    assert not earliest.any() and np.array_equal(before, after)
    none, priced_only, same = planner.balance(n, ops, masks, np.zeros(len(masks)), COSTS, place=False)
    assert none is None and np.array_equal(priced_only, before) and np.array_equal(same, before)


def test_short_batches_count_their_own_passes():
    """a batch that rule (d) shrinks from two ops to one runs as ONE pass: `pass_count` is the kept lists', batch by batch"""
    n = 12
    RY, Z, H = orc.gate_matrix("RY", {"theta": 0.7}), orc.gate_matrix("Z"), orc.gate_matrix("H")
    two = [([5], RY), ([5], Z)]
    assert len(planner.rewrite_ops(n, two, None, COSTS)) == 1
    long_list = device_cases(n)[0][2]
    batches = [planner.rewrite_ops(n, ops) for ops in (two, long_list, [([3], H)])]
    priced = [planner.rewrite_ops(n, ops, None, COSTS) for ops in (two, long_list, [([3], H)])]
    masks = [planner.search_tiles(n, ops) if len(ops) >= 2 else np.zeros(0, dtype=np.uint64) for ops in batches]
    kept, placed, split = engine.priced_variant(n, batches, priced, masks, COSTS)
    want = sum(planner.pass_count(n, ops, ms, pl) if len(ops) >= 2 else len(ops) for ops, ms, pl in zip(kept, masks, placed))
    assert split["pass_count"] == want, split
