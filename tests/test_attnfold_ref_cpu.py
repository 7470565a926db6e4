"""The reference of tests/test_attnfold_abi_gpu.py checked on the CPU: tests/_attnfold_ref.py against the module
arithmetic it restates, the preconditions of the exact cases of tests/_attnfold_cases.py, the gates of the random cases
measured from the reference alone, and the teeth - every deliberate mistake of _attnfold_ref.MUTATIONS moves the
compared quantity of every family it can reach by ten gates, or a bit where the family is compared bit for bit.

Measured here (one fp32 evaluation of the rounded chain against the fp64 one; rel-L2, largest |delta| / max|ref|):
    random_B2_M32_N64 1.31e-5 1.77e-4 | random_B2_M20_N33_strided 3.10e-5 3.24e-4 | random_B3_M32_N200_scale0.25 1.75e-5
    1.51e-4 | random_B1_M7_N1 4.7e-8 5.4e-8        ->  GATES rel_l2 1.24e-4, max_rel 1.32e-3
and the rounded reference against the unrounded module arithmetic on the same operands (where the 2e-2 / 5e-2 budget of
tests/test_attnfold_gpu.py goes): rel-L2 7.7e-4 to 1.2e-3, largest |delta| / max|ref| 1.1e-3 to 2.1e-3 - the rest of
that budget is the rounding of X and Y themselves, which both sides here share.
"""
import numpy as np
import pytest
import torch

import _attnfold_cases as K
import _attnfold_ref as R
from _stack_ref import bf16


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", K.RANDOM, ids=[c.id for c in K.RANDOM])
def test_unrounded_reference_is_the_module_attention(case):
    """rounded=False against nn.MultiheadAttention's core as tests/test_attnfold_gpu.py writes it out, with any key bias
    (constant along the keys).  That formula has 1/sqrt(32) built in; another scale goes into the queries."""
    from test_attnfold_gpu import _ref
    d = K.attn_inputs(case)
    B, M, N = case.B, case.M, case.N
    t = lambda a, *s: torch.from_numpy(np.array(a, np.float64)).reshape(*s)
    bk = torch.randn(256, generator=torch.Generator().manual_seed(case.seed), dtype=torch.float64)
    want = _ref(t(d["q"], B, M, 256) * (case.scale * 32 ** 0.5), t(d["X"], B, N, 256), t(d["Y"], B, N, 256), t(d["wk"], 256, 256),
                bk, t(d["wv"], 256, 256), t(d["bv"], 256), 8).reshape(B * M, 256).numpy()
    got = K.attn_reference(case, rounded=False)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_perm_image_is_the_stated_permutation():
    """The permutation of test_cast_perm_bf16_is_the_stated_permutation (tests/test_attnfold_gpu.py), which pins the
    device's image bit for bit."""
    p = torch.arange(16)
    chan = (p & 3) | ((p & 4) << 1) | ((p & 8) >> 1)
    index = (torch.arange(0, 256, 16).view(16, 1) + chan.view(1, 16)).reshape(256).numpy()
    rows = np.random.default_rng(0).standard_normal((5, 256))
    assert np.array_equal(R.perm_image(rows), rows[:, index])
    assert np.array_equal(R.unperm_image(R.perm_image(rows)), rows)
    assert not np.array_equal(R.perm_image(rows), rows)


def test_bf16_bits_round_trip():
    a = bf16(np.random.default_rng(1).standard_normal(1000))
    assert np.array_equal(R.from_bits16(R.bits16(a)), a)
    assert np.array_equal(R.bits16(a), torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------ the exact cases
EXACT = K.ONEHOT + K.UNIFORM


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_exact_attention_cases_hold_their_preconditions(case):
    """The builder asserts margin >= 160 for every (b, h, q), the winners' spread, l = N and integer sums <= 255
    (_attnfold_cases.check_exact_preconditions).  Here: the rounded reference IS the closed form, and stays so in one
    fp32 evaluation to a thousandth of the elementwise gate."""
    d = K.attn_inputs(case)                    # asserts
    o, det = K.attn_reference(case, details=True)
    assert np.array_equal(det["mag"], d["mag"])
    assert np.abs(o - d["expect"]).max() <= 1e-13 * d["mag"].max()
    if case.family == "onehot":
        assert (det["l"] == 1.0).all() and float(K.margins(case, d, det["S"]).min()) >= K.MARGIN
    o32 = K.attn_reference(case, accumulate=np.float32)
    assert (np.abs(o32 - d["expect"]) <= 1e-3 * K.EXACT_GATE * d["mag"]).all()


def test_onehot_cases_cover_every_tile_edge():
    assert sorted({c.N for c in K.ONEHOT}) == [1, 31, 32, 33, 64, 65, 97, 129] and {c.M for c in K.ONEHOT} == {32, 7}
    assert K.special_keys(129) == [0, 31, 32, 63, 64, 95, 96, 127, 128] and K.special_keys(32) == [0, 31]
    assert sorted({c.N for c in K.UNIFORM}) == [1, 31, 33, 65, 85]


@pytest.mark.parametrize("case", K.POSMEM_EXACT, ids=[c.id for c in K.POSMEM_EXACT])
def test_exact_posmem_cases_are_integers_and_the_reference_has_their_bits(case):
    case = case.resolved(K.CPU_CUS)
    d = K.posmem_inputs(case)
    combos = []
    for b0_on, b2_on, x, y in K.posmem_exact_expected(d):                # asserts h in {0..3}, integers below 256
        combos.append((b0_on, b2_on))
        rx, ry = K.posmem_reference(case, b0_on, b2_on)
        assert np.array_equal(R.bits16(rx), R.bits16(R.perm_image(x))) and np.array_equal(R.bits16(ry), R.bits16(R.perm_image(y)))
        rx32, ry32 = K.posmem_reference(case, b0_on, b2_on, accumulate=np.float32)
        assert np.array_equal(rx32, rx) and np.array_equal(ry32, ry)
    assert combos == K.BIAS_COMBOS


# ------------------------------------------------------------------------------------------ the gates
def test_the_gates_follow_from_what_one_fp32_evaluation_costs():
    """FIGURES are re-measured (the rounded chain in one fp32 evaluation against the fp64 one, per random case), and the
    committed GATES must be 4 x the largest, within 10 %.  A gate above 5e-3 would mean a rounding is missing from the
    restatement."""
    fig = {}
    for case in K.RANDOM:
        ref, _ = K.random_reference(case)
        fig[case.id] = K.errors(ref, K.attn_reference(case, accumulate=np.float32))
        print(f"FIGURE {case.id} rel_l2={fig[case.id][0]:.3e} max_rel={fig[case.id][1]:.3e}")
    assert set(fig) == set(K.FIGURES)
    for i, name in enumerate(("rel_l2", "max_rel")):
        want = 4.0 * max(v[i] for v in fig.values())
        assert abs(K.GATES[name] - want) <= 0.1 * want, (name, K.GATES[name], want)
        assert K.GATES[name] <= 5e-3
        assert K.GATES[name] == 4.0 * max(v[i] for v in K.FIGURES.values())


@pytest.mark.parametrize("case", K.RANDOM, ids=[c.id for c in K.RANDOM])
def test_the_roundings_stay_inside_the_config5_budget(case):
    """rounded=True against rounded=False on the same stored operands: inside the 2e-2 / 5e-2 of
    test_folded_attention_against_fp64, and far above the gates - the two tests ask different questions."""
    ref, _ = K.random_reference(case)
    rel, mx = K.errors(K.attn_reference(case, rounded=False), ref)
    print(f"ROUNDINGS {case.id} rel_l2={rel:.3e} max_rel={mx:.3e}")
    assert rel < 2e-2 and mx < 5e-2
    assert rel > K.GATES["rel_l2"]


@pytest.mark.parametrize("case", K.POSMEM_RANDOM, ids=[c.id for c in K.POSMEM_RANDOM])
def test_the_x16_rule_holds_on_the_references_own_fp32_evaluation(case):
    """The rule of the random posmem cases is a condition, not a share: the fp32 evaluation never breaks it, y16 is
    bit-equal, and the elements the rule could excuse are under 1 % of all."""
    x, y, det = K.posmem_reference(case, details=True)
    x32, y32 = K.posmem_reference(case, accumulate=np.float32)
    bad, differ, inside, need = R.x16_rule(det["pre"], det["mag"], R.unperm_image(x32), K.X16_DELTA)
    wide = R.x16_rule(det["pre"], det["mag"], R.unperm_image(x32), 2.0 ** -15)[2]
    print(f"X16 {case.id} differ={differ} of {x.size} inside={inside / x.size:.4f} (at 2^-15: {wide / x.size:.4f}) "
          f"needed delta=2^{np.log2(need) if need else -np.inf:.1f}")
    assert bad == 0 and np.array_equal(y32, y)
    assert inside < K.X16_SHARE * x.size
    assert R.x16_rule(det["pre"], det["mag"], R.unperm_image(x), K.X16_DELTA)[:2] == (0, 0)


# ------------------------------------------------------------------------------------------ teeth
def _attn_move(case, mutation):
    """How far the mutated reference is from what the family compares against, in gates (inf: not finite)."""
    got = K.attn_reference(case, mutation=mutation)
    if case.family == "random":
        ref, _ = K.random_reference(case)
        rel, mx = K.errors(ref, got)
        return min(rel / K.GATES["rel_l2"], mx / K.GATES["max_rel"])          # both figures must move
    d = K.attn_inputs(case)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - d["expect"]) / (K.EXACT_GATE * d["mag"])).max())


def _posmem_move(case, mutation):
    """1 where the mutated images fail the family's comparison on some bias combination, else 0."""
    case = case.resolved(K.CPU_CUS)
    grid = min(-(-case.rows // 256), K.CPU_CUS)
    for b0_on, b2_on in (K.BIAS_COMBOS if case.family == "posmem_exact" else [(True, True)]):
        x, y, det = K.posmem_reference(case, b0_on, b2_on, details=True)
        mx, my = K.posmem_reference(case, b0_on, b2_on, mutation=mutation, grid=grid)
        same = lambda a, b: np.array_equal(a, b)                              # NaN (never written) differs from anything
        if case.family == "posmem_exact":
            if not (same(mx, x) and same(my, y)):
                return 1
        elif R.x16_rule(det["pre"], det["mag"], R.unperm_image(mx), K.X16_DELTA)[0] or not same(my, y):
            return 1
    return 0


PAIRS = [(f, m) for f in K.FAMILIES for m in R.MUTATIONS if K.applies(f, m)]
CASES_OF = dict(onehot=K.ONEHOT, uniform=K.UNIFORM, random=K.RANDOM, posmem_exact=K.POSMEM_EXACT, posmem_random=K.POSMEM_RANDOM)


@pytest.mark.parametrize("family,mutation", PAIRS, ids=[f"{f}-{m}" for f, m in PAIRS])
def test_every_mutation_bites_every_family_it_can_reach(family, mutation):
    """At least one case of the family sees the mistake at ten gates (one differing bit in the bit-exact families).  A
    pair listed in CANNOT_BITE must, on the contrary, stay inside one gate on every case: the reason given is checked,
    not taken on trust."""
    attn = K.FAMILIES[family] == "attn"
    moves = {c.id: (_attn_move if attn else _posmem_move)(c, mutation) for c in CASES_OF[family]}
    need = 10.0 if attn else 1
    bitten = [k for k, v in moves.items() if not v < need]
    print(f"TEETH {family} {mutation}: bites {len(bitten)} of {len(moves)} cases, largest move {max(moves.values()):.3g}")
    if (family, mutation) in K.CANNOT_BITE:
        assert all(v < 1.0 for v in moves.values()), (K.CANNOT_BITE[(family, mutation)], moves)
    else:
        assert bitten, moves


def test_the_table_of_mutations_is_complete():
    assert set(R.MUTATIONS) == {"last_key_dropped", "last_key_doubled", "tail_unmasked", "no_swap", "wv_next_head",
                                "bv_next_head", "no_bv", "scale_ignored", "no_log2e", "no_b2", "y_from_mempos", "tile_skipped"}
    assert all((f, m) in PAIRS for f, m in K.CANNOT_BITE)
    # a mistake of one kernel cannot reach the cases of the other; no_swap reaches both
    assert sorted(m for m in R.MUTATIONS if K.applies("onehot", m) and K.applies("posmem_exact", m)) == ["no_swap"]
