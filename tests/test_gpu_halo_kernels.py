"""The halo exchange kernels at production halo sizes, on all three transports, against a numpy model.

What moves a halo (csrc/vector.hip, csrc/window.hip) and where its structure changes with the number n of entries.
The figures are read off ``ew_blocks`` (256 threads, one entry per thread and pass, at most 2 048 blocks),
``put_blocks`` (256 threads, WBATCH = 8 entries per thread and pass, 2 048 entries per block, at most 256 blocks) and
``window_exchange_whole`` (1 024 threads, 8 entries per thread and pass, 4 096 entries per block chosen from
max(n_send, n_recv), at most 64 blocks) as they stand; a retuning of those constants moves the cases below.

  pack_kernel / unpack_kernel / unpack_add_kernel (callbacks) and pack_pos_kernel / unpack_pos_kernel /
  unpack_add_pos_kernel (RCCL staging, 32-double padding of every segment): ceil(n / 256) blocks, one pass up to
  2 048 * 256 = 524 288 entries, a grid-stride second pass above.
      n = 1, 255: one block, partly filled; 2 048: 8 full blocks; 2 049 ... 66 049: 9 ... 259 blocks with a tail;
      524 288: 2 048 full blocks, exactly one pass; 524 289, 600 001: second pass of 1 / 75 713 entries.

  window_put_kernel, window_get_kernel<false>, window_get_kernel<true> (split exchange): ceil(n / 2 048) blocks.
      n = 1, 255: one block (no count-in), batch slots clamped to n - 1 and masked; 2 048: one block, every slot of
      the one pass in range; 2 049, 4 096: 2 blocks -- the count-in on L_PACK_DONE / L_UNPACK_DONE, last block raises
      the flags and resets the counter; 4 097: 3 blocks; 16 641: 9; 66 049: 33; 524 288: 256 blocks, one full pass;
      524 289, 600 001: 256 blocks and a second pass of the WBATCH loop (1 / 75 713 entries).

  window_exchange_kernel (one launch: put, then get, one grid for both): ceil(max(n_send, n_recv) / 4 096) blocks,
  a pass covers 8 192 entries per block.
      n <= 4 096: one block; 4 097: 2 blocks (count-in of both phases inside one launch); 16 641: 5; 66 049: 17;
      524 288: 64 blocks, one full pass; 524 289, 600 001: 64 blocks and a second pass.
      Two ranks with (70 146, 4) entries: 18 blocks, of which 17 have nothing to get on the rank that sends the
      face (and nothing to put on the other) -- and 35 blocks against one in the split kernels.

Every comparison is on the bytes of the whole vector (owned entries outside the send list, ghosts that nobody
sends, -0.0 and NaN sentinels included).  The data are integer-valued doubles below 2^20 in magnitude, new for every
exchange, so sums are exact in any order and the model ``ref[n_local + recv] = x[send]`` /
``np.add.at(ref, send, x[n_local + recv])`` is compared with equality; one pass per layout runs standard-normal
data (forward bit-exact; reverse bit-exact where an owned index occurs at most once, within k * 2^-53 * sum|terms|
where it occurs k times: the first-order bound of a (k + 1)-term sum in any order).

The rank is its own neighbour (one process, one stream, nothing to wait for), or -- the last test -- two processes
share the GPU and really wait for each other.  Graph replays go through ``torch.cuda.graph`` on a side stream.
"""
import functools
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 2048, 2049, 4096, 4097, 16641, 66049, 524288, 524289, 600001)
SPARE = 5  # ghosts that no segment receives
LIM = 1 << 20


def _counts(n, k):
    """n entries over k segments: k = 3 unequal, odd where n allows it; k = 4 the same with an empty segment."""
    if k == 1:
        return (n,)
    a, b = (n // 7) | 1, (n // 2) | 1
    c = n - a - b
    assert c > 0 and len({a, b, c}) == 3
    return (a, b, c) if k == 3 else (a, 0, b, c)


def _cases():
    out = []
    for n in SIZES:
        ks = [1] + ([3] if n >= 4097 else []) + ([4] if n == 66049 else [])
        for k in ks:
            for variant in ("distinct", "repeated"):
                if variant == "repeated" and n < 255:
                    continue  # (nothing to repeat)
                out.append(pytest.param(n, k, variant, id=f"{n}-k{k}-{variant}"))
    return out


class _Plan:
    pass


@functools.lru_cache(maxsize=None)
def _plan(n, k, variant):
    """Send and receive lists of one layout (computed once, shared by the transports, read-only).
    distinct: n different owned dofs.  repeated: about a tenth of the owned dofs of the list appear two or three
    times, at random places -- in several segments, inside one block and across blocks -- as edge and corner dofs
    do.  The receive list is a scrambled choice of n of the n + SPARE ghosts."""
    rng = np.random.default_rng(1000 * k + n + (7 if variant == "repeated" else 0))
    d2, d3 = (n // 16, n // 32) if variant == "repeated" else (0, 0)
    u = n - d2 - 2 * d3
    p = _Plan()
    p.n, p.counts = n, _counts(n, k)
    p.n_local = u + max(8, u // 16) + 3
    owned = rng.permutation(p.n_local)[:u]
    send = np.concatenate([owned, owned[:d2], owned[d2:d2 + d3], owned[d2:d2 + d3]])
    rng.shuffle(send)
    p.send = send.astype(np.int32)
    p.ghosts = n + SPARE
    p.recv = rng.permutation(p.ghosts)[:n].astype(np.int32)
    p.total = p.n_local + p.ghosts
    assert 8 * p.total < 10_000_000
    p.occurs = np.bincount(p.send, minlength=p.n_local)
    assert (p.occurs.max() == 3 and (p.occurs == 2).any()) if d3 else p.occurs.max() == (2 if d2 else 1)
    p.unsent = np.nonzero(p.occurs == 0)[0]
    p.unreceived = np.setdiff1d(np.arange(p.ghosts), p.recv)
    assert p.unsent.size >= 8 and p.unreceived.size == SPARE
    for a in (p.send, p.recv, p.occurs, p.unsent, p.unreceived):
        a.setflags(write=False)
    return p


_SENTINELS = np.array([0x7FF8_0000_0000_BEEF, 0x8000_0000_0000_0000, 0x7FF0_0000_0000_0000, 0xFFF8_0000_0000_0001,
                       0x0000_0000_0000_0001], dtype=np.uint64).view(np.float64)  # NaN, -0.0, inf, -NaN, denormal


def _fresh(p, rng, normal=False):
    """A whole vector of new values; entries the exchange must leave alone carry bit patterns that `==` would not
    tell apart (or not find equal): the ghosts nobody sends and five owned entries outside the send list."""
    x = rng.standard_normal(p.total) if normal else rng.integers(-LIM + 1, LIM, p.total).astype(np.float64)
    x[p.n_local + p.unreceived] = _SENTINELS
    x[p.unsent[:5]] = _SENTINELS[::-1]
    return x


def _forward_model(p, x):
    ref = x.copy()
    ref[p.n_local + p.recv] = x[p.send]
    return ref


def _reverse_model(p, x):
    ref = x.copy()
    np.add.at(ref, p.send, x[p.n_local + p.recv])
    return ref


def _difference(got, ref, where=None):
    """None, or where the bytes of two vectors first differ."""
    a, b = got.view(np.uint64), ref.view(np.uint64)
    ne = a != b
    if where is not None:
        ne &= where
    if not ne.any():
        return None
    i = int(np.nonzero(ne)[0][0])
    return f"{int(ne.sum())} entries differ, the first at {i}: got {got[i]!r} ({int(a[i]):#018x}), expected {ref[i]!r} ({int(b[i]):#018x})"


class _SelfComm:
    """Callbacks transport of a rank that is its own neighbour: what was packed is what arrives."""

    native = None
    distributed = True
    rank, world = 0, 1

    def exchange(self, L, phase):
        if phase == 0:
            L.recv_buffer[: L.n_recv].copy_(L.send_buffer[: L.n_send])
        elif phase == 2:
            L.send_buffer[: L.n_send].copy_(L.recv_buffer[: L.n_recv])

    def allreduce(self, L, host, op):
        pass


@pytest.fixture(scope="module")
def pm(built):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pmg_dolfinx_amd as pm

    torch.cuda.set_device(0)
    return pm


@pytest.fixture(scope="module")
def transport(request, pm):
    """(name, communicator): "callbacks", "rccl" (the library's communicator, padded staging buffers) or "windows"."""
    name = request.param
    if name == "callbacks":
        comm = _SelfComm()
    else:
        comm = pm.RcclComm(0, 1, pm.RcclComm.unique_id(), halo="windows" if name == "windows" else "exchange")
    yield name, comm
    del comm
    gc.collect()


def _one_cell_operator(pm, layout):
    """A degree-1 operator of one cell over the first eight owned dofs, no dof marked: its apply_lifting is the
    layout's whole forward exchange and nothing else."""
    part = pm.BoxPartition((1, 1, 1))
    lv = part.level(1)
    return pm.MatFreeLaplacian(1, 1.0, lv.dofmap, part.xgeom, part.geom_dofmap, np.zeros(1, np.int32),
                               np.zeros(0, np.int32), np.zeros(layout.total, np.int8), layout)


class _Exchanger:
    """One layout with its vectors; every step uploads a new vector, runs one exchange and compares all of it."""

    def __init__(self, pm, p, comm, windows):
        import torch

        self.pm, self.p, self.torch = pm, p, torch
        self.layout = pm.Layout(p.n_local, p.ghosts, [0] * len(p.counts), p.counts, p.counts, p.send.copy(),
                                p.recv.copy(), comm=comm)
        self.x, self.w = pm.Vector(self.layout), pm.Vector(self.layout)
        self.w.set(1.0)
        self.between = 0
        self.op = self.b = None
        if windows:
            self.op, self.b = _one_cell_operator(pm, self.layout), pm.Vector(self.layout)

    def upload(self, a):
        self.x.data.copy_(self.torch.from_numpy(a))

    def forward_split(self):
        self.x.scatter_fwd_begin()
        self.pm.scale(self.w, 2.0)  # an unrelated vector kernel between begin and end, as the interior cells are
        self.between += 1
        self.x.scatter_fwd_end()

    def reverse_split(self):
        self.x.scatter_rev_begin()
        self.x.scatter_rev_end()

    def forward_whole(self):
        self.op.apply_lifting(self.x, self.b)

    def step(self, kind, a, what):
        before = self.layout.forward_scatters()
        self.upload(a)
        {"F": self.forward_split, "R": self.reverse_split, "W": self.forward_whole}[kind]()
        got = self.x.data_copy()
        assert self.layout.forward_scatters() - before == (0 if kind == "R" else 1)
        ref = _reverse_model(self.p, a) if kind == "R" else _forward_model(self.p, a)
        bad = _difference(got, ref)
        assert bad is None, f"{what}: {bad}"

    def bystanders_untouched(self):
        assert np.array_equal(self.w.data_copy(), np.full(self.p.total, 2.0 ** self.between))
        if self.b is not None:
            assert not self.b.data_copy().view(np.uint64).any()  # no cell touches a marked dof: b is never written


@pytest.mark.parametrize("n,k,variant", _cases())
@pytest.mark.parametrize("transport", ["callbacks", "rccl", "windows"], indirect=True)
def test_self_neighbour_exchanges_match_the_model(pm, transport, n, k, variant):
    name, comm = transport
    p = _plan(n, k, variant)
    windows = name == "windows"
    ex = _Exchanger(pm, p, comm, windows)
    rng = np.random.default_rng(n + k)
    if windows:
        assert ex.op.lift_cell_count() == -1
        ex.step("W", _fresh(p, rng), "first apply_lifting")  # builds the operator's host list: outside the sequence
        assert ex.op.lift_cell_count() == 0
    # twelve exchanges, more than the two window slots: slot reuse and the reset of the count-in counters
    sequence = "FRWFWRRFWWRF" if windows else "FRFFFRRFFFRF"
    for i, kind in enumerate(sequence):
        ex.step(kind, _fresh(p, rng), f"exchange {i} ({kind}) of {sequence}")
    # standard-normal data, once each way
    a = _fresh(p, rng, normal=True)
    ex.step("W" if windows else "F", a, "forward, normal data")
    if windows:
        ex.step("F", _fresh(p, rng, normal=True), "forward split, normal data")
    ex.upload(a)
    ex.reverse_split()
    got = ex.x.data_copy()
    ref = _reverse_model(p, a)  # one rounding where an index occurs once: the same bits
    once = np.ones(p.total, dtype=bool)
    once[: p.n_local] = p.occurs <= 1
    bad = _difference(got, ref, where=once)
    assert bad is None, f"reverse, normal data: {bad}"
    many = np.nonzero(p.occurs > 1)[0]
    if many.size:
        terms = a[p.n_local + p.recv].astype(np.longdouble)
        exact, mag = a[: p.n_local].astype(np.longdouble), np.abs(a[: p.n_local]).astype(np.longdouble)
        np.add.at(exact, p.send, terms)
        np.add.at(mag, p.send, np.abs(terms))
        err = np.abs(got[many].astype(np.longdouble) - exact[many])
        bound = p.occurs[many] * np.longdouble(2.0 ** -53) * mag[many]
        worst = int(np.argmax(err - bound))
        print(f"reverse, normal data: max error / bound {float((err / bound).max()):.3f} over {many.size} repeated dofs")
        assert (err <= bound).all(), (int(many[worst]), float(err[worst]), float(bound[worst]))
    ex.bystanders_untouched()


@pytest.mark.parametrize("n", [66049, 4097])
@pytest.mark.parametrize("transport", ["rccl", "windows"], indirect=True)
def test_captured_exchanges_replay_with_new_values(pm, transport, n):
    """One forward exchange captured with torch.cuda.graph on a side stream (after an eager one: peer connections
    and the operator's host list are set up outside a capture), replayed five times with new owner values; on the
    windows both forms, split and whole.  The exchange number lives on the device, so every replay is a new exchange
    in the other window slot."""
    import torch

    name, comm = transport
    windows = name == "windows"
    p = _plan(n, 3, "repeated")
    rng = np.random.default_rng(n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ex = _Exchanger(pm, p, comm, windows)
        ex.step("F", _fresh(p, rng), "eager split")
        forms = {"F": ex.forward_split}
        if windows:
            ex.step("W", _fresh(p, rng), "eager whole")
            forms["W"] = ex.forward_whole
        side.synchronize()
        for kind, issue in forms.items():
            before = ex.layout.forward_scatters()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
                issue()
            assert ex.layout.forward_scatters() == before + 1  # counted once, at capture
            for rep in range(5):
                a = _fresh(p, rng)
                ex.upload(a)
                graph.replay()
                side.synchronize()
                bad = _difference(ex.x.data_copy(), _forward_model(p, a))
                assert bad is None, f"replay {rep} of the captured {kind} exchange: {bad}"
            assert ex.layout.forward_scatters() == before + 1
            del graph
        # ... and the layout goes on exchanging eagerly behind the replays
        ex.step("R", _fresh(p, rng), "eager reverse after the replays")
        ex.step("F", _fresh(p, rng), "eager split after the replays")
        side.synchronize()
    del ex


# ---------------------------------------------------------------------------------------------------------------
# Two processes on the one GPU: the sides of the exchange differ in block count and wait for each other.
PAIR_COUNTS = ((66049, 0, 4097), (3, 0, 1))  # what rank 0 sends (= rank 1 receives) and receives (= rank 1 sends)
PAIR_SEQUENCE = "FRWFWRRFWWRF"


def _pair_plan(rank):
    """The halo plan of `rank` (both ranks compute both).  Rank 0 sends a face with repeated dofs and an edge in
    segments 0 and 2 and receives four entries; rank 1 mirrors it.  Segment j of one rank pairs with segment j of
    the other (HaloWindows: the j-th time a rank appears in a list)."""
    rng = np.random.default_rng(40 + rank)
    send_counts, recv_counts = PAIR_COUNTS if rank == 0 else PAIR_COUNTS[::-1]
    ns, nr = sum(send_counts), sum(recv_counts)
    p = _Plan()
    p.send_counts, p.recv_counts = send_counts, recv_counts
    if rank == 0:
        d2, d3 = ns // 16, ns // 32
        u = ns - d2 - 2 * d3
        p.n_local = u + u // 16 + 11
        owned = rng.permutation(p.n_local)[:u]
        send = np.concatenate([owned, owned[:d2], owned[d2:d2 + d3], owned[d2:d2 + d3]])
        rng.shuffle(send)
    else:
        p.n_local = 64
        send = rng.permutation(p.n_local)[:ns]
        send[-1] = send[0]  # the one entry of segment 2 is a dof of segment 0 as well
    p.send = send.astype(np.int32)
    p.ghosts = nr + SPARE
    p.recv = rng.permutation(p.ghosts)[:nr].astype(np.int32)
    p.total = p.n_local + p.ghosts
    return p


def _pair_data(rank, e, p):
    """Integer data that encode (rank, exchange number, position)."""
    return (((2 * e + rank) << 20) + np.arange(p.total, dtype=np.int64)).astype(np.float64)


def _pair_body(rank, world, port, route):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("PMG_WINDOW_TIMEOUT_MS", "20000")  # the ranks time-slice one GPU: generous, still bounded
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pmg_dolfinx_amd as pm

        torch.cuda.set_device(0)
        if route == "windows-split":
            os.environ["PMG_FUSED_EXCHANGE"] = "0"
        comm = pm.TorchComm(halo="windows")
        me, peer = _pair_plan(rank), _pair_plan(1 - rank)
        layout = pm.Layout(me.n_local, me.ghosts, [1 - rank] * 3, me.send_counts, me.recv_counts, me.send, me.recv,
                           comm=comm)
        op, b = _one_cell_operator(pm, layout), pm.Vector(layout)
        out = {"mismatches": [], "exchanges": 0}

        def expected(kind, e):
            mine, theirs = _pair_data(rank, e, me), _pair_data(1 - rank, e, peer)
            if kind == "R":
                np.add.at(mine, me.send, theirs[peer.n_local + peer.recv])
            else:
                mine[me.n_local + me.recv] = theirs[peer.send]
            return mine

        def issue(kind, x):
            before = layout.forward_scatters()
            if kind == "F":
                x.scatter_fwd_begin()
                pm.scale(b, 1.0)  # an unrelated vector kernel between begin and end
                x.scatter_fwd_end()
            elif kind == "R":
                x.scatter_rev_begin()
                x.scatter_rev_end()
            else:
                op.apply_lifting(x, b)
            assert layout.forward_scatters() - before == (0 if kind == "R" else 1)

        def run(kinds, first):
            # every exchange on a vector of its own, all issued before the first is looked at: no host barrier and
            # no synchronisation in between, the ranks drift as far as the protocol lets them
            xs = []
            for i in range(len(kinds)):
                x = pm.Vector(layout)
                x.data.copy_(torch.from_numpy(_pair_data(rank, first + i, me)))
                xs.append(x)
            for kind, x in zip(kinds, xs):
                issue(kind, x)
            torch.cuda.synchronize()
            for i, (kind, x) in enumerate(zip(kinds, xs)):
                bad = _difference(x.data_copy(), expected(kind, first + i))
                if bad is not None:
                    out["mismatches"].append(f"rank {rank}, exchange {first + i} ({kind}): {bad}")
            out["exchanges"] += len(kinds)

        assert op.lift_cell_count() == -1
        run("W", 0)  # the first apply_lifting builds a host list (and synchronises)
        assert op.lift_cell_count() == 0
        run(PAIR_SEQUENCE, 1)
        run(PAIR_SEQUENCE[::-1], 1 + len(PAIR_SEQUENCE))  # data regenerated; the exchange numbers go on
        out["b_untouched"] = not b.data_copy().view(np.uint64).any()
        dist.barrier()  # nobody frees a window a neighbour may still acknowledge into
        return out
    finally:
        dist.destroy_process_group()


def _pair_worker(rank, world, port, *rest):
    from test_gpu_distributed import _reporting

    _reporting(_pair_body)(rank, world, port, *rest)


def test_two_processes_with_unequal_sides(built):
    """Rank 0 sends 70 146 entries in segments (66 049, 0, 4 097) and receives (3, 0, 1); rank 1 the mirror image.
    Rank 0 puts with 35 blocks and gets with one, its one-launch kernel has 18 blocks of which 17 have nothing to
    get; in reverse rank 0 adds 70 146 values, repeated dofs among them, with 35 blocks counting in.  One pair of
    processes per route, the second route only after the first has passed.  (PMG_FUSED_EXCHANGE=0 governs which
    form an operator or a transfer chooses; apply_lifting asks for the whole exchange on either route, so the
    one-launch kernel runs between two processes on both.)"""
    import torch

    from test_gpu_distributed import _run_ranks

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for route in ("windows", "windows-split"):
        res = _run_ranks(_pair_worker, 2, (route,))
        for out in res:
            assert not out["mismatches"], (route, out["mismatches"][:4])
            assert out["exchanges"] == 1 + 2 * len(PAIR_SEQUENCE) and out["b_untouched"], (route, out)
