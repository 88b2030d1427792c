"""The checker of the fused all-reduce jobs' values (tests/comm_checker.py) is
not vacuous: a CPU emulation of the exchange (receive regions, parity slots,
flags, one-shot and two-shot, write-G and Adam epilogues) passes it on the
synthetic arena for s = 2, 3, 4, 8 over four epochs, and each mutated
emulation -- a wrong reduce the suite could not see before, because every test
with more than one rank fed equal or only replica-compared contributions --
fails it. The conditions on the inputs that make the mutants visible are
asserted too. Mutants live in the emulation only; no mutated kernel exists."""
import pytest
import torch

from tests import comm_checker as cc
from tests import conv_small_checker as ck

SIZES = (2, 3, 4, 8)
HP = ck.ADAM_SETS["coupled"]


def _run(s, two, mutant=None, mode="push|reduce", hp=None, epochs=cc.EPOCHS, first_only=False):
    emu = cc.ExchangeEmu(s, 1.0 / s, two_shot=two, mutant=mutant)
    fails = []
    for e in epochs:
        cc.run_epoch(emu, e, mode, hp)
        fails += cc.check_emu(emu, e, hp)
        if fails and first_only:
            break
    return fails


# --------------------------------------------------------------- the table ----
def test_arena_table_is_in_the_domain_and_reaches_every_path():
    assert cc.NUMEL % 4 == 0
    counts = {c for _, _, c in cc.UNITS}
    assert counts >= {1, 3, 37, 255, 256, 257, 258, 1021, 1023, 1024}
    assert sorted({ns for _, _, ns in cc.SEGS}) == [0, 1, 3, 20]
    for si, (off, n, ns) in enumerate(cc.SEGS):
        assert off % 4 == 0 and n % 4 == 0
        mine = [(st, c) for s_, st, c in cc.UNITS if s_ == si]
        assert {c for _, c in mine} == counts          # every count in every kind of segment
        for st, c in mine:
            assert 0 <= st and st + c <= n             # no unit crosses its segment
            assert c <= cc.THREADS or (off + st) % 4 == 0
    gap = int((~cc.MASK).sum())
    assert gap >= 4 * len(cc.SEGS) + cc.SEG_GAP * (len(cc.SEGS) - 1)
    # the two-shot arithmetic of the table
    assert cc.chunk_sizes(32, 3) == [12, 12, 8]                                   # a ragged last chunk
    assert cc.chunk_sizes(1, 3) == [1, 0, 0] and cc.chunk_sizes(1, 4) == [1, 0, 0, 0]   # owners without a chunk
    assert cc.chunk_sizes(3, 4) == [3, 0, 0, 0]
    for s in (3, 4):                                   # a vec4 unit's chunk boundary inside the unit
        ch = cc.two_shot_chunk(1021, s)
        assert 0 < ch < 1021 and ch % 4 == 0 and sum(cc.chunk_sizes(1021, s)) == 1021
        assert cc.chunk_sizes(1021, s)[-1] not in (0, ch)


def test_own_sum_is_the_documented_order():
    """Independent route: numpy float32 accumulators written out per element
    for one vec4 element (one lane of slab_sum4 == slab_sum1) and one scalar
    column (slab_partial + the row sum)."""
    import numpy as np

    g = ck.gen(3)
    f = np.float32
    for ns in (1, 3, 20):
        slab = torch.randn(ns, 300, generator=g)
        x = slab.numpy()
        a = [f(0)] * 4
        q = ns // 4
        for i in range(q):
            for j in range(4):
                a[j] = f(a[j] + x[4 * i + j, 299])
        for k in range(4 * q, ns):
            a[0] = f(a[0] + x[k, 299])
        want = f(f(0) + f(f(a[0] + a[1]) + f(a[2] + a[3])))
        assert cc.own_sum(slab, 300)[299].item() == want
        cnt, rp = 37, 256 // 37
        rows = []
        for rl in range(rp):
            a = [f(0)] * 4
            s_ = rl
            while s_ + 3 * rp < ns:
                for j in range(4):
                    a[j] = f(a[j] + x[s_ + j * rp, 5])
                s_ += 4 * rp
            while s_ < ns:
                a[0] = f(a[0] + x[s_, 5])
                s_ += rp
            rows.append(f(f(a[0] + a[1]) + f(a[2] + a[3])))
        want = f(0)
        for r in rows:
            want = f(want + r)
        assert cc.own_sum(slab[:, :cnt], cnt)[5].item() == want


# ------------------------------------------- conditions on the inputs ----
def test_inputs_make_order_and_scaling_visible():
    for s in SIZES:
        own, red = cc.expected(s, 1, 1.0 / s)
        rev = cc.reverse_ref(own, 1.0 / s)
        pre = cc.reduce_ref([g * torch.tensor(1.0 / s) for g in own], 1.0)
        m = cc.MASK
        if s == 2:
            assert torch.equal(rev[m], red[m])          # order cannot be seen at s = 2
        else:
            assert cc.frac_differ(rev[m], red[m]) >= 0.10, s
        if s == 3:
            assert cc.frac_differ(pre[m], red[m]) >= 0.10
        else:
            assert torch.equal(pre[m], red[m])          # 1/s a power of two: exact
        for r in range(s):                              # a rank's own gradient is not the mean
            assert cc.frac_differ(own[r][m], red[m]) >= 0.5


# ------------------------------------------------ the unmutated emulation ----
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("s", SIZES)
def test_emulation_passes(s, two):
    assert _run(s, two) == []
    assert _run(s, two, mode="push+reduce", hp=HP) == []


def test_push_check():
    emu = cc.ExchangeEmu(3, 1.0 / 3)
    own, _ = cc.expected(3, 2, 1.0 / 3)
    for r in range(3):
        emu.load(r, *cc.rank_data(r, 2))
        for k in range(len(cc.UNITS)):
            emu.push(r, k, 2)
        assert cc.check_push(emu.G[r], own[r]) == []
    bad = cc.ExchangeEmu(3, 1.0 / 3, mutant="push_arena_for_slab")
    bad.load(0, *cc.rank_data(0, 2))
    for k in range(len(cc.UNITS)):
        bad.push(0, k, 2)
    assert cc.check_push(bad.G[0], own[0]), cc.MUTANTS["push_arena_for_slab"]


def test_a_reduce_ahead_of_its_producer_is_reported():
    emu = cc.ExchangeEmu(2, 0.5)
    for r in range(2):
        emu.load(r, *cc.rank_data(r, 1))
    emu.push(0, 0, 1)
    with pytest.raises(cc.WouldWait):
        emu.reduce(0, 0, 1)


# ------------------------------------------------------------- the mutants ----
# mutant -> (group sizes, two-shot forms, Adam epilogue)
CASES = {
    "peer_slot_plus_one": ((2, 3, 4), (False, True), False),
    "drop_last_double_first": ((2, 3, 8), (False, True), False),
    "reverse_order": ((3, 4, 8), (False, True), False),
    "prescale": ((3,), (False, True), False),
    "stale_parity": ((2, 3), (False, True), False),
    "chunk_not_rounded": ((3,), (True,), False),
    "nonowner_keeps_partial": ((3, 4), (True,), False),
    "adam_own": ((2, 3), (False, True), True),
    "push_arena_for_slab": ((2, 3), (False, True), False),
}


def test_every_mutant_has_a_case():
    assert set(CASES) == set(cc.MUTANTS)


@pytest.mark.parametrize("mutant", list(CASES))
def test_mutant_fails_the_checker(mutant):
    sizes, forms, adam = CASES[mutant]
    for s in sizes:
        for two in forms:
            fails = _run(s, two, mutant=mutant, hp=HP if adam else None, first_only=mutant != "stale_parity")
            assert fails, f"mutant not seen at s = {s}, two_shot = {two}: {cc.MUTANTS[mutant]}"
            if mutant == "stale_parity":
                # fresh data every epoch: once both slots were written the stale one holds real (finite)
                # values of an earlier epoch, and the checker still sees them
                assert any("epoch 3" in f for f in fails) and any("epoch 4" in f for f in fails), \
                    cc.MUTANTS[mutant]


def test_stale_parity_reads_finite_values_from_epoch_3():
    emu = cc.ExchangeEmu(2, 0.5, mutant="stale_parity")
    for e in cc.EPOCHS:
        cc.run_epoch(emu, e)
        if e >= 3:
            assert bool(torch.isfinite(emu.G[0][cc.MASK]).all())
            assert cc.check_emu(emu, e), cc.MUTANTS["stale_parity"]
