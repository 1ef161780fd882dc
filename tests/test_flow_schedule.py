"""Host logic of the dataflow Cholesky (csrc/cholflow.hip): the task list every form of the factorisation runs from.
No device needed: the list is built on the host.  The test replays the list in ticket order next to a model of the chain
kernel's workgroups and checks what the kernels rely on (cholflow.hip, "Order and progress"):

  * a ticket only ever waits for tiles of EARLIER tickets or for the chain kernel's workgroups, which in turn only wait for
    earlier tickets (no deadlock whatever the residency);
  * every tile of the lower triangle (and of the right-hand-side rows) gets every block-column update exactly once -- from
    the tile kernel or from the chain workgroup the form assigns it to -- and is finished exactly once, after all of them.
"""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_amd import engine

FIN = 1 << 20


PART, NPART_SHIFT, BUF_SHIFT = 1 << 21, 22, 12


def tasks(nb, rows, w, chain, second=0, split_m=1, split_from=1 << 30):
    lib = engine.load_library()
    lib.jaicov_debug_flow_tasks2.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_int]
    n = lib.jaicov_debug_flow_tasks2(nb, rows, w, chain, second, split_m, split_from, None, 0)
    assert n > 0
    out = np.zeros((n, 4), np.int32)
    assert lib.jaicov_debug_flow_tasks2(nb, rows, w, chain, second, split_m, split_from, out.ctypes.data, n) == n
    return out


class Replay:
    def __init__(self, nb, rows, chain, second):
        self.nb, self.rows, self.chain, self.second = nb, rows, chain, second
        self.done = np.zeros((rows, nb), bool)       # L[i][k] final (done[k][k]: the inverse too)
        self.stored = np.zeros((rows, nb), bool)     # the tile is in memory ...
        self.applied = np.zeros((rows, nb), int)     # ... with that many block columns subtracted
        self.updates = np.zeros((rows, nb), int)
        self.factored = np.zeros(nb, bool)
        self.c0 = 0          # workgroup 0: next block column
        self.c2 = 0          # workgroup 2: next block column
        self.half2 = False   # workgroup 2 has finished tile (c2+2, c2), its update of (c2+2, c2+1) is still to come

    def has(self, i, j, k):
        return self.stored[i, j] and self.applied[i, j] == k

    def chain_kernel(self):
        """potrf_chain_kernel's workgroups, as far as what is in memory lets them go."""
        nb = self.nb
        moved = True
        while moved:
            moved = False
            c = self.c0
            if c < nb and not self.factored[c]:      # workgroup 0: potrf(c); tile (0, 0) from memory, the others are in its LDS
                if c > 0 or self.has(0, 0, 0):
                    self.factored[c] = moved = True
            if c < nb and self.factored[c]:
                if c + 1 >= nb:
                    self.c0 = nb
                elif self.has(c + 1, c, c) and self.has(c + 1, c + 1, c):
                    self.done[c + 1, c] = True       # L[c+1][c] by forward substitution
                    self.updates[c + 1, c + 1] += 1  # ... subtracted from the next diagonal tile, which stays in LDS
                    self.c0 = c + 1
                    moved = True
            for k in range(nb):                      # workgroup 1: the inverses
                if self.factored[k] and not self.done[k, k]:
                    self.done[k, k] = moved = True
            if self.second >= 1:
                c = self.c2
                if c + 2 < nb and self.factored[c]:
                    if not self.half2 and self.has(c + 2, c, c):
                        self.done[c + 2, c] = True
                        self.half2 = moved = True
                    if self.half2:
                        if self.second < 2:
                            self.c2, self.half2, moved = c + 1, False, True
                        elif self.has(c + 2, c + 1, c) and self.done[c + 1, c]:
                            self.updates[c + 2, c + 1] += 1
                            self.applied[c + 2, c + 1] = c + 1
                            self.c2, self.half2, moved = c + 1, False, True

    def run(self, t):
        psum = {}                                    # partial-sum buffer -> (tile, block columns it holds)
        for (i, j, z, wd) in t:
            k0, buf = int(z) & ((1 << BUF_SHIFT) - 1), int(z) >> BUF_SHIFT
            k1, fin = int(wd) & (FIN - 1), bool(int(wd) & FIN)
            part, npart = bool(int(wd) & PART), (int(wd) >> NPART_SHIFT) & 7
            assert 0 <= j <= i < self.rows and j < self.nb and 0 <= k0 <= k1 <= j
            if self.chain:
                self.chain_kernel()
            for k in range(k0, k1):                  # operands: final by now
                assert self.done[i, k] and self.done[j, k], ("ticket would wait for a later ticket", i, j, k)
            if part:                                 # a partial sum of a split range: its own buffer, written once
                assert not fin and npart == 0 and buf not in psum and k1 > k0
                psum[buf] = ((i, j), k0, k1)
                continue
            if npart > 0:                            # the tile's own task: first visit, the last piece, + the partial sums of EARLIER tickets
                assert not self.stored[i, j]
                at = 0
                for q in range(npart):
                    assert buf + q in psum, "the partial sum comes from an earlier ticket"
                    tile, a, b = psum.pop(buf + q)
                    assert tile == (i, j) and a == at, "the pieces tile the range"
                    self.updates[i, j] += b - a
                    at = b
                assert at == k0
            elif k0 > 0:
                assert self.has(i, j, k0), "a later visit continues where the earlier one stopped"
            else:
                assert not self.stored[i, j]
            self.updates[i, j] += k1 - k0
            self.stored[i, j] = True
            self.applied[i, j] = k1
            if fin:
                assert k1 == j, "a tile is finished after ALL its updates"
                if i == j:
                    assert not self.chain
                    self.done[j, j] = True           # the diagonal kernel / inline
                else:
                    if self.chain:
                        self.chain_kernel()
                    assert self.done[j, j], ("the inverse this ticket waits for cannot be there yet", i, j)
                    self.done[i, j] = True
        if self.chain:
            self.chain_kernel()
        assert not psum, "every partial sum is added exactly once"


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 29, 118])
@pytest.mark.parametrize("form", [(0, 0), (1, 0), (1, 1), (1, 2)])
@pytest.mark.parametrize("w", [1, 4])
def test_task_list_is_complete_and_deadlock_free(nb, form, w):
    chain, second = form
    rows = nb + 1                                    # + the right-hand-side row block
    r = Replay(nb, rows, chain, second)
    r.run(tasks(nb, rows, w, chain, second))
    low = np.tril(np.ones((rows, nb), bool))
    assert r.done[low].all(), "every tile of the lower triangle is finished"
    want = np.tile(np.arange(nb), (rows, 1))
    assert (r.updates[low] == want[low]).all(), "every tile gets each block-column update exactly once"


@pytest.mark.parametrize("nb", [20, 47, 118, 142])
@pytest.mark.parametrize("form", [(0, 0), (1, 0), (1, 2)])
@pytest.mark.parametrize("split", [(2, 0), (2, None), (3, 30), (8, 0)])
def test_split_update_ranges_keep_the_list_complete_and_deadlock_free(nb, form, split):
    """Round 5: the tasks of the late block columns hand part of their update range to partial-sum tasks (cholflow.hip, FLOW_PART).  Same
    guarantees: operands only from earlier tickets, every update exactly once, every partial sum added exactly once by its tile's own task."""
    chain, second = form
    m, frm = split
    if frm is None:                                  # the solver's own rule
        lib = engine.load_library()
        a, b = C.c_int(0), C.c_int(0)
        lib.jaicov_debug_flow_split(nb, C.byref(a), C.byref(b))
        m, frm = a.value, b.value
        assert (m, frm) == ((2, nb // 2) if nb >= 80 else (1, 1 << 30))
    rows = nb + 1
    t = tasks(nb, rows, 1, chain, second, m, frm)
    plain = tasks(nb, rows, 1, chain, second)
    n_part = int(((t[:, 3] & PART) != 0).sum())
    assert len(t) == len(plain) + n_part and (n_part > 0) == (m > 1 and nb - 1 >= max(8 * m, frm))
    r = Replay(nb, rows, chain, second)
    r.run(t)
    low = np.tril(np.ones((rows, nb), bool))
    assert r.done[low].all()
    want = np.tile(np.arange(nb), (rows, 1))
    assert (r.updates[low] == want[low]).all()


def layout(nb, rows, partials):
    lib = engine.load_library()
    lib.jaicov_debug_flow_layout.argtypes = [C.c_int] * 3 + [C.c_void_p]
    out = np.zeros(8, np.int64)
    max_grid = lib.jaicov_debug_flow_layout(nb, rows, partials, out.ctypes.data)
    assert max_grid > 0
    return [int(x) for x in out], max_grid


def default_split_partials(nb, rows):
    lib = engine.load_library()
    m, frm = C.c_int(0), C.c_int(0)
    lib.jaicov_debug_flow_split(nb, C.byref(m), C.byref(frm))
    t = tasks(nb, rows, 1, 1, 0, m.value, frm.value)
    return int(((t[:, 3] & PART) != 0).sum())        # two pieces: one partial-sum buffer per split task


def test_flag_layout_is_one_disjoint_cover_and_matches_the_kernels_arithmetic(monkeypatch):
    """The flag words of the dataflow factorisation (cholflow.h, FlowLayout): the host fills the kernel's pointers, sizes and clears the
    allocation and reads the stall report from ONE layout.  Its offsets are those the factorisation has always used (written out here)."""
    monkeypatch.delenv("JAICOV_FLOW_SPLIT", raising=False)
    p118 = default_split_partials(118, 119)
    assert p118 > 0
    CTRL = 16
    for nb, rows, p in [(1, 2, 0), (24, 25, 0), (118, 119, p118)]:
        (done, applied, diag_ready, factored, wgstate, wgsnap, pflag, total), max_grid = layout(nb, rows, p)
        sizes = [rows * nb, rows * nb, nb, nb, max_grid, max_grid, p]
        starts = [done, applied, diag_ready, factored, wgstate, wgsnap, pflag]
        # the regions follow the control words, in order, without gap or overlap, and end at the total
        assert done == CTRL
        for q in range(7):
            assert starts[q] + sizes[q] == (starts[q + 1] if q < 6 else total), (nb, q)
        # the offsets the factorisation used before there was a layout
        assert done == 16
        assert applied == 16 + rows * nb
        assert diag_ready == 16 + 2 * rows * nb
        assert factored == 16 + 2 * rows * nb + nb
        assert wgstate == 16 + 2 * rows * nb + 2 * nb
        assert pflag == 16 + 2 * rows * nb + 2 * nb + 2048
        assert total == 16 + 2 * rows * nb + 2 * nb + 2048 + p
        # the snapshot of the state words (flow_give_up) lies FLOW_MAX_GRID words after them
        assert wgsnap == wgstate + max_grid and max_grid == 1024


HOOKS = ["JAICOV_FACTOR_FORM", "JAICOV_FLOW_MIN_BLOCKS", "JAICOV_FLOW_SPLIT", "JAICOV_FLOW_TIMEOUT_MS", "JAICOV_FLOW_TRACE_ON",
         "JAICOV_CHAIN8_MIN_NB", "JAICOV_CHAIN_TRACE", "JAICOV_VERBOSE"]
NO_SPLIT = (1, 1 << 30)
# (form hook, block columns, kernels overlap) -> (dataflow, one kernel, chain form, third chain workgroup, split pieces, first split column)
DECISIONS = [
    (None, 6, True, (0, 0, 0, 0) + NO_SPLIT),            # below 12 block columns: the stream-scheduled factorisation
    (None, 11, True, (0, 0, 0, 0) + NO_SPLIT),
    (None, 12, True, (1, 0, 1, 2) + NO_SPLIT),           # chain form, third chain workgroup below 80 block columns
    (None, 29, True, (1, 0, 1, 2) + NO_SPLIT),
    (None, 79, True, (1, 0, 1, 2) + NO_SPLIT),
    (None, 80, True, (1, 0, 1, 0, 2, 40)),               # from 80 on: two chain workgroups, update ranges split from the middle column on
    (None, 118, True, (1, 0, 1, 0, 2, 59)),
    ("streams", 29, True, (0, 0, 0, 0) + NO_SPLIT),
    ("streams", 118, True, (0, 0, 0, 0, 2, 59)),
    ("two_step", 29, True, (1, 0, 0, 0) + NO_SPLIT),
    ("two_step", 118, True, (1, 0, 0, 0, 2, 59)),
    ("one_kernel", 29, True, (1, 1, 0, 0) + NO_SPLIT),
    ("chain2", 29, True, (1, 0, 1, 0) + NO_SPLIT),
    ("chain3", 29, True, (1, 0, 1, 2) + NO_SPLIT),
    ("chain3", 118, True, (1, 0, 1, 2, 2, 59)),
    (None, 29, False, (1, 1, 0, 0) + NO_SPLIT),          # kernels cannot run side by side: one kernel, whatever the form
    (None, 118, False, (1, 1, 0, 0, 2, 59)),
    ("chain3", 29, False, (1, 1, 0, 0) + NO_SPLIT),
    (None, 6, False, (0, 0, 0, 0) + NO_SPLIT),
]


@pytest.mark.parametrize("form,nb,overlap,want", DECISIONS)
def test_the_form_of_the_factorisation_is_decided_in_one_place(monkeypatch, form, nb, overlap, want):
    """Which factorisation a solver uses (cholflow.h, flow_decide): the first four columns are what the solver did when the rule was spread
    over DenseSolver::init and flow_init (zeros where it never got as far as asking, the stream-scheduled form); the last two are the split
    rule, which was a function of the block columns and its hook alone (flow_split_rule behind jaicov_debug_flow_split), whatever the form."""
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    if form is not None:
        monkeypatch.setenv("JAICOV_FACTOR_FORM", form)
    lib = engine.load_library()
    out = (C.c_int * 6)()
    lib.jaicov_debug_flow_decision(nb, int(overlap), out)
    assert tuple(out) == want


def test_the_hooks_reach_the_decision(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    lib = engine.load_library()
    out = (C.c_int * 6)()
    monkeypatch.setenv("JAICOV_FLOW_MIN_BLOCKS", "1")
    monkeypatch.setenv("JAICOV_FLOW_SPLIT", "3:30")
    lib.jaicov_debug_flow_decision(6, 1, out)
    assert tuple(out) == (1, 0, 1, 2, 3, 30)
    monkeypatch.setenv("JAICOV_FLOW_SPLIT", "0")         # fewer than one piece: one
    lib.jaicov_debug_flow_decision(6, 1, out)
    assert tuple(out) == (1, 0, 1, 2, 1, 0)


# (block columns, right-hand sides, compute units) -> (polling-wave form, workgroups per block column, right-hand sides the kernel carries)
CHAIN_DECISIONS = [
    (None, (23, 1, 256), (0, 1, 1)),         # below 24 block columns: backsolve_chain_kernel<1>
    (None, (24, 1, 256), (1, 2, 1)),         # the polling-wave form, two workgroups per block column while the grid is resident at once
    (None, (128, 1, 256), (1, 2, 1)),
    (None, (129, 1, 256), (1, 1, 1)),        # 2 nb > compute units: one workgroup per block column
    (None, (24, 1, 0), (1, 1, 1)),           # the compute units could not be asked
    (None, (24, 2, 256), (0, 1, 2)),         # more than one right-hand side: backsolve_chain_kernel<2 / 4 / 8>
    (None, (24, 3, 256), (0, 1, 4)),
    (None, (24, 4, 256), (0, 1, 4)),
    (None, (24, 5, 256), (0, 1, 8)),
    (None, (24, 8, 256), (0, 1, 8)),
    ("1", (1, 1, 256), (1, 1, 1)),           # JAICOV_CHAIN8_MIN_NB=1: the split form still only from 8 block columns on
    ("1", (7, 1, 256), (1, 1, 1)),
    ("1", (8, 1, 256), (1, 2, 1)),
    ("1", (8, 2, 256), (0, 1, 2)),
]


def chain_decision(nb, nrhs, cus):
    lib = engine.load_library()
    out = (C.c_int * 3)()
    lib.jaicov_debug_chain_decision(nb, nrhs, cus, out)
    return tuple(out)


@pytest.mark.parametrize("min_nb,case,want", CHAIN_DECISIONS)
def test_the_form_of_the_substitution_chains_is_decided_in_one_place(monkeypatch, min_nb, case, want):
    """Which chain kernels a substitution launches (chains.h, chain_decide): what the solver did when the rule was written out in
    DenseSolver::backsolve_aug, solve_rhs and chain8_split (pre-multiplied blocks and exchange vector present; an MI355X reports 256
    compute units)."""
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    if min_nb is not None:
        monkeypatch.setenv("JAICOV_CHAIN8_MIN_NB", min_nb)
    assert chain_decision(*case) == want


def test_the_chain_hook_is_read_at_every_call(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    monkeypatch.setenv("JAICOV_CHAIN8_MIN_NB", "1")
    assert chain_decision(8, 1, 256) == (1, 2, 1)
    monkeypatch.delenv("JAICOV_CHAIN8_MIN_NB")
    assert chain_decision(8, 1, 256) == (0, 1, 1)
