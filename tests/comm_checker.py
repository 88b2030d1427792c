"""Shared oracle of the fused all-reduce jobs (csrc/kernels/comm_jobs.h,
``comm_unit_body``) with MORE THAN ONE rank holding different gradients: the
reference values, a synthetic arena, a checker of what a rank's arenas hold
after a push / a reduce / a reduce + Adam, and a CPU emulation of the exchange
whose mutants show that the checker is not vacuous
(tests/unit/test_comm_checker.py). The GPU tests
(tests/gpu/test_comm_jobs_values.py and its workers) hand the same checker the
kernel's arenas.

What is bitwise and why:

* The own contribution of a unit (push): the split-K slab sum in the finalize
  order of conv_small.h (``own_sum``): ``rp = 256 // count`` row lanes for
  ``count <= 256``, else 4 elements per thread. A vec4 thread with fewer than
  4 elements left uses ``slab_sum1``, whose order is that of one lane of
  ``slab_sum4`` (four interleaved accumulators over the slabs, the remainder
  into the first, ``0 + ((a0 + a1) + (a2 + a3))``): the same per element as
  ``rp = 1``. A slab-free segment's contribution is the arena value itself.
* The reduce: ``acc = g_0; acc = acc + g_1; ...`` in rank order in float32,
  then ``acc * float32(scale)`` (``reduce_ref``). One-shot and two-shot alike:
  the two-shot owner of a chunk forms the same sum and the others copy it.
  Add-then-scale holds no multiply-add for a compiler to contract.
* Adam in the reduce's epilogue is compared within ``adam_ref``'s own bounds
  (tests/conv_small_checker.py) on the expected gradient, its bf16 twin
  bitwise; with Adam the arena keeps the own contribution.

Inputs: standard-normal slabs and arena values from ``(rank, epoch)`` seeds,
fresh every epoch, so a stale parity slot, a wrong peer or a wrong order shows
in the values (the unit test asserts the fractions of elements that do).
"""

from __future__ import annotations

import numpy as np
import torch

from tests import conv_small_checker as ck

POISON = -12345.0          # arena elements no unit owns: exactly representable, never produced
BF16 = torch.bfloat16
THREADS = 256              # kFinalizeThreads

# --------------------------------------------------------------- the arena ----
# Slab counts of the four segments (0 = no slabs: the gradient is already in
# G; 20 is past the 16-slab batched-load path) and the unit counts laid out in
# EACH of them: the scalar path's edges (1, 3, 37, 255, 256: rp = 256, 85, 6,
# 1, 1), vec4 units with ragged tails of 1, 2, 1 and 3 elements (257, 258,
# 1021, 1023), a full vec4 unit (1024) and a 32-element unit (two-shot chunks
# 12 / 12 / 8 at s = 3). A vec4 unit starts on a multiple of 4 (16-B stores);
# the elements skipped for that, 4 elements at each segment's end and the
# elements between the segments belong to no unit.
SEG_SLABS = (0, 1, 3, 20)
UNIT_COUNTS = (1024, 1021, 257, 1023, 258, 256, 255, 37, 32, 3, 1)
SEG_GAP = 8


def _layout():
    segs, units, off = [], [], 4
    for si, ns in enumerate(SEG_SLABS):
        cur = 0
        for c in UNIT_COUNTS:
            if c > THREADS:
                cur = (cur + 3) // 4 * 4
            units.append((si, cur, c))
            cur += c
        n = (cur + 3) // 4 * 4 + 4
        segs.append((off, n, ns))
        off += n + SEG_GAP
    return tuple(segs), tuple(units), off


SEGS, UNITS, NUMEL = _layout()   # (off, numel, nslabs) | (seg, start, count) | arena elements
assert NUMEL % 4 == 0 and all(o % 4 == 0 and n % 4 == 0 for o, n, _ in SEGS)
EPOCHS = (1, 2, 3, 4)            # both receive parities, twice


def unit_range(u):
    si, st, c = u
    o0 = SEGS[si][0] + st
    return o0, o0 + c


def unit_mask() -> torch.Tensor:
    m = torch.zeros(NUMEL, dtype=torch.bool)
    for u in UNITS:
        a, b = unit_range(u)
        assert not bool(m[a:b].any()), "units overlap"
        m[a:b] = True
    return m


MASK = unit_mask()


def two_shot_chunk(count: int, s: int) -> int:
    return ((count + s - 1) // s + 3) // 4 * 4


def chunk_sizes(count: int, s: int):
    """Elements of a unit owned by rank 0 .. s-1 in the two-shot form."""
    ch = two_shot_chunk(count, s)
    return [max(0, min(count, (q + 1) * ch) - q * ch) for q in range(s)]


_DATA, _OWN = {}, {}


def rank_data(rank: int, epoch: int):
    """Cached ``_rank_data``: the tensors are shared, never written."""
    if (rank, epoch) not in _DATA:
        _DATA[(rank, epoch)] = _rank_data(rank, epoch)
    return _DATA[(rank, epoch)]


def _rank_data(rank: int, epoch: int):
    """(G0 [NUMEL], slabs {seg: [ns, seg numel]}) of one rank in one epoch:
    standard normal from the (rank, epoch) seed; POISON outside the units. A
    segment with slabs still gets an arena value (never to be read)."""
    g = ck.gen(100_003 * epoch + 17 * rank + 5)
    G0 = torch.randn(NUMEL, generator=g)
    G0[~MASK] = POISON
    slabs = {si: torch.randn(ns, n, generator=g) for si, (_, n, ns) in enumerate(SEGS) if ns}
    return G0, slabs


def adam_state(epoch: int):
    """P, m, v planted equally on every rank (conv_small_checker.adam_inputs)."""
    p, _, m, v = ck.adam_inputs(NUMEL, seed=7 + epoch)
    return p, m, v


# ----------------------------------------------------------------- oracles ----
def _emulated_sum(slab, rp):
    """The finalize kernel's summation order in float32 (conv_small.h): thread
    row rl sums slabs rl, rl + rp, ... into 4 interleaved accumulators (full
    quads, the remainder into the first), then row 0 adds the rp row sums in
    order starting from 0."""
    ns = slab.shape[0]
    z = torch.zeros(slab.shape[1], dtype=torch.float32)
    g = z.clone()
    for rl in range(rp):
        ks = list(range(rl, ns, rp))
        a = [z.clone() for _ in range(4)]
        q = len(ks) // 4
        for i in range(q):
            for j in range(4):
                a[j] = a[j] + slab[ks[4 * i + j]]
        for k in range(4 * q, len(ks)):
            a[0] = a[0] + slab[ks[k]]
        g = g + ((a[0] + a[1]) + (a[2] + a[3]))
    return g


def own_sum(slabs, count: int):
    """One unit's finalize: ``slabs`` [ns, count] f32 -> [count] f32, in the
    kernel's order (scalar units: rp = 256 // count row lanes; vec4 units and
    their one-element tails: one lane, rp = 1)."""
    assert slabs.shape[1] == count
    return _emulated_sum(slabs, THREADS // count if count <= THREADS else 1)


def reduce_ref(contribs, scale: float):
    """Rank-order float32 sum of the contributions, then x float32(scale)."""
    acc = contribs[0].clone()
    for g in contribs[1:]:
        acc = acc + g
    return acc * torch.tensor(np.float32(scale))


def reverse_ref(contribs, scale: float):
    return reduce_ref(list(contribs)[::-1], scale)


def own_contribution(rank: int, epoch: int):
    """What rank's arena holds after its pushes of the epoch ([NUMEL] f32)."""
    G0, slabs = rank_data(rank, epoch)
    g = G0.clone()
    for si, st, c in UNITS:
        off, _, ns = SEGS[si]
        if ns:
            g[off + st:off + st + c] = own_sum(slabs[si][:, st:st + c], c)
    return g


_EXPECT = {}


def expected(s: int, epoch: int, scale: float):
    """(own [s][NUMEL], reduced [NUMEL]); the reduced arena keeps POISON
    outside the units. Computed once per (s, epoch, scale) and shared."""
    key = (s, epoch, float(np.float32(scale)))
    if key not in _EXPECT:
        own = [own_contribution(r, epoch) for r in range(s)]
        red = reduce_ref(own, scale)
        red[~MASK] = POISON
        _EXPECT[key] = (own, red)
    return _EXPECT[key]


# ----------------------------------------------------------------- checker ----
def check_push(G, own) -> list:
    """After a rank's pushes: its arena is its own contribution, bitwise."""
    bad = int((G != own).sum())
    return [f"push: {bad} elements differ from own_sum"] if bad else []


def check_reduce(G, red) -> list:
    """After a rank's reduces without Adam: the arena is the rank-order sum x
    scale on the units and POISON elsewhere, bitwise."""
    out = []
    bad = int((G[MASK] != red[MASK]).sum())
    if bad:
        out.append(f"reduce: {bad} of {int(MASK.sum())} unit elements differ from reduce_ref")
    if not bool((G[~MASK] == POISON).all()):
        out.append("reduce: an element outside every unit was written")
    return out


def check_adam(P, G, m, v, w16, own, red, p0, m0, v0, c) -> (list, dict):
    """After a rank's reduces with Adam (constants ``c``: ck.adam_consts):
    P, m, v within adam_ref's bounds of one step on the EXPECTED gradient, w16
    the bitwise bf16 twin of P, G still the own contribution, nothing written
    outside the units. Returns (failures, {name: largest error / bound})."""
    out, ratios = [], {}
    rp, rm, rv, bp, bm, bv = ck.adam_ref(p0[MASK], red[MASK], m0[MASK], v0[MASK], c)
    for name, got, ref, bound in (("P", P, rp, bp), ("m", m, rm, bm), ("v", v, rv, bv)):
        ratios[name] = r = ck.ratio(got[MASK], ref, bound)
        if not r <= 1:
            out.append(f"adam: {name} error / bound {r:.4g}")
    if not torch.equal(w16[MASK], P[MASK].to(BF16)):
        out.append("adam: w16 is not the bf16 rounding of P")
    if int((G != own).sum()):
        out.append("adam: G no longer holds the own contribution")
    for name, got, init in (("P", P, p0), ("m", m, m0), ("v", v, v0)):
        if not torch.equal(got[~MASK], init[~MASK]):
            out.append(f"adam: {name} written outside the units")
    if not bool((w16[~MASK].float() == ck.BF16_FILL).all()):
        out.append("adam: w16 written outside the units")
    return out, ratios


# ----------------------------------------------- emulation of the exchange ----
MUTANTS = {
    "peer_slot_plus_one": "peer slot (p + 1) % s read in place of p",
    "drop_last_double_first": "the last rank left out and rank 0 counted twice",
    "reverse_order": "the sum taken in reverse rank order",
    "prescale": "contributions scaled before the sum",
    "stale_parity": "the reduce of epoch e reads parity (e - 1) & 1",
    "chunk_not_rounded": "the two-shot chunk is not rounded up to 4 (by the pushing side)",
    "nonowner_keeps_partial": "a two-shot non-owner keeps its own partial sum",
    "adam_own": "Adam is fed the own contribution in place of the reduced one",
    "push_arena_for_slab": "the push takes the arena value for a segment that has slabs",
}


class WouldWait(RuntimeError):
    """A reduce was asked for before the flags it waits for were published."""


class ExchangeEmu:
    """s ranks, receive regions [2 parity][s src][NUMEL] per rank (NaN until
    written: the kernel's region is not initialised either), one flag per
    (src, unit) stored at the unit's first element; the steps of
    ``comm_unit_body`` on the table above, one unit of one rank at a time.

    ``reduce`` is the reduce up to the owner's sum (one-shot: every element is
    its rank's own; two-shot: the owner's chunk, sent to every peer, flag 2e);
    ``finish`` picks up the other owners' chunks (two-shot) and runs the
    epilogue: write G, or Adam with the bf16 twin when ``adam`` (constants of
    ck.adam_consts) is given. ``mutant`` = a key of MUTANTS."""

    def __init__(self, s, scale, two_shot=False, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.s, self.scale, self.mutant = s, torch.tensor(np.float32(scale)), mutant
        self.two = bool(two_shot) and s > 2
        nan = float("nan")
        self.recv = [torch.full((2, s, NUMEL), nan) for _ in range(s)]
        self.flags = [torch.zeros(s, NUMEL, dtype=torch.int64) for _ in range(s)]
        self.G = [torch.full((NUMEL,), POISON) for _ in range(s)]
        self.slabs = [None] * s
        self.P = self.m = self.v = self.w16 = None
        self._g, self._acc = {}, {}

    def load(self, rank, G0, slabs):
        self.G[rank], self.slabs[rank] = G0.clone(), slabs
        self._g.clear()

    def plant_adam(self, p, m, v):
        self.P = [p.clone() for _ in range(self.s)]
        self.m = [m.clone() for _ in range(self.s)]
        self.v = [v.clone() for _ in range(self.s)]
        self.w16 = [torch.full((NUMEL,), ck.BF16_FILL, dtype=BF16) for _ in range(self.s)]

    # a unit's elements owned by rank q (arena index tensors); one-shot: all are `me`'s
    def _owned(self, u, q, me, pushing=False):
        a, b = unit_range(u)
        if not self.two:
            return torch.arange(a, b) if q == me else torch.arange(0)
        c = u[2]
        ch = two_shot_chunk(c, self.s)
        if pushing and self.mutant == "chunk_not_rounded":
            ch = (c + self.s - 1) // self.s
        return torch.arange(a + min(c, q * ch), a + min(c, (q + 1) * ch))

    def _own(self, rank, u, push):
        si, st, c = u
        a, b = unit_range(u)
        if push and SEGS[si][2] and self.mutant != "push_arena_for_slab":
            key = (id(self.slabs[rank][si]), u)   # rank_data's tensors live in _DATA for the process
            if key not in _OWN:
                _OWN[key] = own_sum(self.slabs[rank][si][:, st:st + c], c)
            return _OWN[key].clone()
        return self.G[rank][a:b].clone()

    def push(self, rank, unit, epoch):
        u, par = UNITS[unit], epoch & 1
        a, b = unit_range(u)
        g = self._own(rank, u, True)
        self._g[(rank, unit)] = g
        self.G[rank][a:b] = g
        for p in range(self.s):
            if p == rank:
                continue
            if self.two:
                ix = self._owned(u, p, rank, pushing=True)   # the chunk's owner only
                self.recv[p][par, rank, ix] = g[ix - a]
            else:
                self.recv[p][par, rank, a:b] = g
            self.flags[p][rank, a] = 2 * epoch - 1

    def _wait(self, rank, a, target):
        for p in range(self.s):
            if p != rank and int(self.flags[rank][p, a]) < target:
                raise WouldWait(f"rank {rank} would wait for rank {p}'s flag {target} at element {a}")

    def reduce(self, rank, unit, epoch, pushed=False):
        u, s = UNITS[unit], self.s
        a, b = unit_range(u)
        par = (epoch - 1) & 1 if self.mutant == "stale_parity" else epoch & 1
        g = self._g[(rank, unit)] if pushed else self._own(rank, u, False)
        self._g[(rank, unit)] = g
        self._wait(rank, a, 2 * epoch - 1)
        ix = self._owned(u, rank, rank)
        order = list(range(s))
        if self.mutant == "drop_last_double_first":
            order = [0] + order[:-1]
        if self.mutant == "reverse_order":
            order = order[::-1]
        acc = None
        for p in order:
            q = (p + 1) % s if self.mutant == "peer_slot_plus_one" and p != rank else p
            term = g[ix - a] if q == rank else self.recv[rank][par, q, ix]
            if self.mutant == "prescale":
                term = term * self.scale
            acc = term.clone() if acc is None else acc + term
        if self.mutant != "prescale":
            acc = acc * self.scale
        full = torch.zeros(u[2])          # the kernel's acc registers start at 0
        full[ix - a] = acc
        self._acc[(rank, unit)] = full
        if self.two:
            for p in range(s):
                if p != rank:
                    self.recv[p][epoch & 1, rank, ix] = acc
                    self.flags[p][rank, a] = 2 * epoch

    def finish(self, rank, unit, epoch, adam=None):
        u, s = UNITS[unit], self.s
        a, b = unit_range(u)
        acc, g = self._acc.pop((rank, unit)), self._g.pop((rank, unit))
        if self.two:
            self._wait(rank, a, 2 * epoch)
            for q in range(s):
                if q != rank:
                    ix = self._owned(u, q, rank)
                    acc[ix - a] = g[ix - a] if self.mutant == "nonowner_keeps_partial" else \
                        self.recv[rank][epoch & 1, q, ix]
        if adam is None:
            self.G[rank][a:b] = acc
            return
        feed = g if self.mutant == "adam_own" else acc
        p2, m2, v2, _, _, _ = ck.adam_ref(self.P[rank][a:b], feed, self.m[rank][a:b], self.v[rank][a:b], adam)
        self.P[rank][a:b], self.m[rank][a:b], self.v[rank][a:b] = p2.float(), m2.float(), v2.float()
        self.w16[rank][a:b] = self.P[rank][a:b].to(BF16)

    def push_reduce(self, rank, unit, epoch):
        """One rank's mode-3 job of a unit up to the owner's sum, when every
        peer's push is already there (the emulation runs one rank at a time)."""
        self.push(rank, unit, epoch)
        self.reduce(rank, unit, epoch, pushed=True)


def run_epoch(emu: ExchangeEmu, epoch: int, mode: str = "push|reduce", hp=None):
    """One epoch of the table on fresh (rank, epoch) data. ``mode``:
    "push|reduce" (modes 1 then 2, as the GPU test issues them in one process)
    or "push+reduce" (mode 3: the own contribution stays in registers; the
    emulation still runs every rank's push first, as the flags require).
    ``hp`` = an ADAM_SETS entry for the Adam epilogue (step = epoch)."""
    s, nu = emu.s, len(UNITS)
    adam = None
    if hp is not None:
        adam = ck.adam_consts(hp, epoch)
        emu.plant_adam(*adam_state(epoch))
    for r in range(s):
        emu.load(r, *rank_data(r, epoch))
    for r in range(s):
        for k in range(nu):
            emu.push(r, k, epoch)
    for r in range(s):
        for k in range(nu):
            emu.reduce(r, k, epoch, pushed=(mode == "push+reduce"))
    for r in range(s):
        for k in range(nu):
            emu.finish(r, k, epoch, adam)


def check_emu(emu: ExchangeEmu, epoch: int, hp=None) -> list:
    """The checker on every rank of the emulation after ``run_epoch``."""
    own, red = expected(emu.s, epoch, float(emu.scale))
    out = []
    for r in range(emu.s):
        if hp is None:
            fails = check_reduce(emu.G[r], red)
        else:
            p0, m0, v0 = adam_state(epoch)
            fails, _ = check_adam(emu.P[r], emu.G[r], emu.m[r], emu.v[r], emu.w16[r], own[r], red, p0, m0, v0,
                                  ck.adam_consts(hp, epoch))
        out += [f"rank {r} epoch {epoch}: {f}" for f in fails]
    return out


def frac_differ(a, b) -> float:
    return float((a != b).double().mean())
