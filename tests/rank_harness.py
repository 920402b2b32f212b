"""How the GPU tests run several ranks on the one GPU of a test box: as spawned processes (`_run_ranks`, workers wrapped
by `_reporting`) or as host threads of the test process (`_ThreadWorld`, `_ThreadComm`: the exchange and all-reduce
callbacks of the C ABI).  A plain module, shared by the test files; it holds no test."""
import socket

import numpy as np


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(target, world, args, timeout=300):
    """Spawn `world` processes running target(rank, world, port, *args, q); every worker puts
    (rank, result) or (rank, exception text) on the queue.  Whatever happens -- a worker that dies
    before reporting, a failure reported by one rank while the others sit in a collective -- every
    process is terminated and joined before the test returns, so no rank is left holding the GPU."""
    import queue as _queue

    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        while len(res) < world:
            try:
                rank, out = q.get(timeout=5)
            except _queue.Empty:
                timeout -= 5
                dead = [i for i, p in enumerate(procs) if p.exitcode not in (None, 0) and i not in res]
                if dead:
                    raise AssertionError(f"rank(s) {dead} died without reporting (exit codes "
                                         f"{[procs[i].exitcode for i in dead]})")
                if timeout <= 0:
                    raise AssertionError("timed out waiting for the ranks")
                continue
            if isinstance(out, str):
                raise AssertionError(f"rank {rank} failed:\n{out}")
            res[rank] = out
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [res[r] for r in range(world)]


def _reporting(fn):
    """Worker wrapper: report the traceback instead of dying silently."""
    import functools

    @functools.wraps(fn)
    def wrapped(rank, world, port, *args):
        q = args[-1]
        try:
            q.put((rank, fn(rank, world, port, *args[:-1])))
        except BaseException:  # noqa: BLE001 -- reported to the parent, which fails the test
            import traceback

            q.put((rank, traceback.format_exc()))
            raise

    return wrapped


# ---------------------------------------------------------------------------------------------
# BASELINE config 3's partition -- 2 x 2 x 2 bricks, every rank with 7 neighbours (3 faces, 3 edges,
# 1 corner) -- on the one GPU of the test box: the eight ranks are eight host THREADS of one process
# (the box admits at most 6 processes on its GPU), each with its own HIP stream and its own library
# objects; the exchange callback of the C ABI moves the packed buffers between the ranks' staging
# buffers with stream-ordered device copies.
class _ThreadWorld:
    def __init__(self, n, barrier_timeout=240):
        """``barrier_timeout`` (seconds): how long a rank waits for the others at an exchange or a reduction before
        the barrier breaks and every waiting rank fails."""
        import threading

        self.n = n
        self.barrier = threading.Barrier(n)
        self.barrier_timeout = barrier_timeout
        self.layouts = [dict() for _ in range(n)]
        self.slots = [None] * n

    def wait(self):
        self.barrier.wait(timeout=self.barrier_timeout)


class _ThreadComm:
    native = None
    staged = False
    distributed = True

    def __init__(self, world, rank):
        self.W, self.rank, self.world = world, rank, world.n
        self._count = 0

    def register(self, layout):  # layouts are created in the same order on every rank
        layout._tid = self._count
        self.W.layouts[self.rank][self._count] = layout
        self._count += 1

    def exchange(self, L, phase):
        import torch

        st = torch.cuda.current_stream()
        W = self.W
        if phase in (0, 2):
            fwd = phase == 0
            L._ev_packed = torch.cuda.Event()
            L._ev_packed.record(st)
            W.wait()  # every rank has packed (on its own stream) and published its event
            off = 0
            for i, nb in enumerate(L.neighbors):
                peer = W.layouts[nb][L._tid]
                cnt = (L.recv_counts if fwd else L.send_counts)[i]
                j = peer.neighbors.index(self.rank)
                pc = peer.send_counts if fwd else peer.recv_counts
                assert pc[j] == cnt, "the two sides of a halo plan disagree"
                po_ = sum(pc[:j])
                st.wait_event(peer._ev_packed)
                src = (peer.send_buffer if fwd else peer.recv_buffer)[po_: po_ + cnt]
                dst = (L.recv_buffer if fwd else L.send_buffer)[off: off + cnt]
                dst.copy_(src)
                off += cnt
            L._ev_copied = torch.cuda.Event()
            L._ev_copied.record(st)
        else:
            W.wait()  # every rank has enqueued its copies: nobody repacks a buffer that is still being read
            for nb in L.neighbors:
                st.wait_event(W.layouts[nb][L._tid]._ev_copied)

    def allreduce(self, L, host, op):
        W = self.W
        W.slots[self.rank] = host.copy()
        W.wait()
        vals = np.stack(W.slots)
        tot = vals.max(axis=0) if op == "max" else vals.sum(axis=0)
        W.wait()
        host[:] = tot
