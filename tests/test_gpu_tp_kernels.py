"""The tensor-parallel exchange kernels alone (csrc/woq_comm.hip, csrc/woq_comm_dev.h, the `tp` branch of the XQ GEMV's
epilogue in csrc/woq_gemv_xqs.h), through `woq_probe_comm_allreduce` / `woq_probe_comm_greedy` / `woq_probe_gemv_xq_tp`
/ `woq_probe_comm_set_seq`, against tests/tp_reference.py and tests/xq_reference.py.

The ranks are processes on one GPU, as in tests/test_gpu_tp_device.py (mp.spawn, gloo for the rendezvous only, an
errfile for the tracebacks, `DeviceComm(5008, timeout_ms=10000)`): one spawn per test function runs that function's
cases in sequence; every rank builds every rank's inputs from the same seed, so each rank knows what to expect without
a gather; `comm.status()` must be 0 after every case, and the first failure raises, which ends the spawn (the other
ranks are terminated, nobody goes on issuing collectives on a communicator that lost step). max_elems 5008 is no
multiple of 1024 and larger than most n: the inbox's slot stride differs from the vector length.

Every comparison is exact but the sums of squares, which keep the project's bound (xq_reference.SSQ_REL against the
float64 block sums, on the blocks `_check_ssq` of tests/test_gpu_xq_gemv_kernel.py holds):
  A  plain all-reduce, world 2: buf == (fl32(0) + x_0) + x_1 in numpy fp32, bit for bit (NaN for NaN), at n = 1 .. 5008
     in an order that puts small vectors on a buffer that last carried a large one and back, on N(0, 1) * 2^U(-60, 60),
     on the special values of fp32 addition, and with either rank held back; the sentinel behind buf[n:] stands; the
     digests of every result are equal on both ranks.
  B  XQ-emitting all-reduce: buf as in A; (limbs, u, sx) == xq_reference.encode(fl32(buf * norm_w)) of the kernel's own
     buf; ssq_out against block_ssq(buf); sentinels behind every output, the limb buffer's padding included. The test
     asserts from the reference alone that the wrong norm weight, no norm weight, or sums of squares of buf * norm_w
     would each miss these checks on its inputs.
  C  pushed form: probe_gemv_xq_tp's `out` == probe_gemv_xq's `out`; all-reduce(pushed=1) of it == fl32(out_0 + out_1) of
     the plain probe's outputs of both shards; XQ as in B; the same with pushed=0 from the same partials: the same
     bytes. K picks the GEMV's geometry (asserted through xq_reference.geometry), 16512 is two chained launches of which
     only the last may push (a first launch that pushed would tag the slots with a partial sum of half the K range).
     Ragged N = 40: the GEMV pushes its 40 live columns only, so the pushed all-reduce runs as the plain variant with
     n = 40 — the XQ variant needs n = 48 and, pushed, would wait out its bound for columns 40 .. 47 that no peer ever
     sends; it runs unpushed on the same partials with the dead columns at 0, and gives the same 40 sums.
  D  the sequence number's wrap (0xfffffffd, six collectives, `0xffffffff -> 2`), then a captured graph of one XQ
     all-reduce (n 4096), one plain one (n 1025) and one greedy pick — three collectives, so the buffer parity of each
     alternates between replays — replayed four times on fresh inputs: exact as in A, B and E.
  E  greedy pick: token, log[old pos], pos + 1 and status == tp_reference.greedy_pick, the single-device argmax with the
     lowest-index rule over the gathered row (tests/test_tp_reference_cpu.py holds it to a brute-force argmax): winner
     on either rank, equal maxima across and inside ranks, a rank of -inf under sentinel indices, a rank of NaN, and the
     two no-winner cases, which give token 0 and status bit 2 on both ranks like
     test_no_winner_gives_token_0_and_status_bit_2_in_both_tails asks of the single-GPU tails; n_pairs 1, 24 and 2000.
  F  world 4, plain all-reduce and greedy pick: with four addends the rank order decides the bits (asserted of the
     inputs: the reverse order gives other bits).

Observed (MI355X, one GPU, the ranks as processes on it; wall time of each test function beside
test_tp_world_size_two_device_exchange's 3.6 s in the same run — most of each is the spawn, the rendezvous and the
HIP start-up of the ranks):
  A  2.9 s, 18 cases: every sum bit for bit, subnormal sums kept (no flush to zero), -0 + -0 leaves as +0, the late rank
     is waited for inside the kernel.
  B  2.4 s, 28 cases: every XQ vector bit for bit; sums of squares within the bound on every held block.
  C  4.3 s, 18 shapes x forms, 36 collectives: the pushing GEMV's `out` is the plain one's; pushed and unpushed
     all-reduces give the same bytes, the chained launch (K 16512) included.
  D  2.6 s, 11 cases: the six collectives across 0xffffffff -> 2 and all four replays exact.
  E  2.8 s, 26 cases. On the kernel as it was before this file the first no-winner case fails with token 0x7fffffff,
     status 0 ("every pair NaN" at 24 pairs); tp_greedy_kernel now takes the engine's status word and applies
     argmax_kernel's rule to the merged pair.
  F  3.6 s, 13 cases: four processes' kernels do run concurrently on the one GPU (status 0 throughout); a library built
     to sum in reverse rank order fails "world 4 plain n 1025" with 49 elements off, as the reference predicts.
Perturbed builds, by hand: the all-reduce emitting with the reversed norm weight fails B at "xq n 4096 norm: limbs";
sums of squares of buf * norm_w fail B at "xq n 4096 norm ssq: ssq".
"""
import hashlib
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import tp_reference as T
from tests import xq_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

F32 = np.float32
MAX_ELEMS = 5008
SENT = 777.0
G128, G32A = (128, False, "fp16"), (32, True, "fp32")  # tests/test_gpu_xq_gemv_kernel.py's two sweep forms


# ---- harness -----------------------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, errfile, family):
    try:
        sys.path.insert(0, ROOT)
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(rank if torch.cuda.device_count() >= world else 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from intel_extension_for_transformers_amd.runtime.comm import DeviceComm

        comm = DeviceComm(MAX_ELEMS, timeout_ms=10000)
        assert comm.error is None, comm.error
        ctx = Ctx(rank, world, comm)
        FAMILIES[family](ctx)
        ctx.ranks_hold_the_same_bits()
        if rank == 0:
            print("%s, world %d: %d cases, status 0 after each, the same bits on every rank" % (family, world, ctx.cases))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        with open(errfile, "a") as fh:
            fh.write("rank %d\n%s\n" % (rank, traceback.format_exc()))
        raise


def _spawn(family, world, tmp_path):
    import torch.multiprocessing as mp

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    errfile = str(tmp_path / "errors.txt")
    try:
        mp.spawn(_rank_main, args=(world, port, errfile, family), nprocs=world, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else "(no traceback captured)"
        pytest.fail("a tensor-parallel rank failed:\n" + msg)


class Ctx:
    """one rank's end of a test function: the communicator, the case counter and the digests of what it saw"""

    def __init__(self, rank, world, comm):
        self.rank, self.world, self.comm = rank, world, comm
        self.digest = hashlib.sha256()
        self.cases = 0

    def done(self, what, *results):
        """after every case: the communicator saw no timeout; remember the bytes this rank ended with"""
        st = self.comm.status()
        assert st == 0, "%s: communicator status %d" % (what, st)
        for r in results:
            self.digest.update(np.ascontiguousarray(r).tobytes())
        self.cases += 1

    def ranks_hold_the_same_bits(self):
        import torch.distributed as dist

        seen = [None] * self.world
        dist.all_gather_object(seen, (self.cases, self.digest.hexdigest()))
        assert len(set(seen)) == 1, seen


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random(rng, n):
    return (rng.standard_normal(n) * np.exp2(rng.uniform(-60, 60, n))).astype(F32)


def _xo_buffers(n):
    nb = n // 16
    return (torch.full((L.xq_limb_bytes(n),), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((nb + 4,), SENT, device="cuda"), torch.full((nb + 4,), SENT, device="cuda"))


def _check_xo(xo, n, y32, what):
    """the XQ vector equals encode(y32) bit for bit; nothing behind it was written"""
    nb = n // 16
    limbs, u, sx = (t.cpu().numpy() for t in xo)
    want = X.encode(y32)
    assert np.array_equal(limbs[:nb * 48].view(np.int8).reshape(nb, 3, 16), want[0]), what + ": limbs"
    assert np.array_equal(u[:nb], want[1]) and np.array_equal(sx[:nb], want[2]), what + ": u / sx"
    assert (limbs[nb * 48:] == 0x5A).all() and (u[nb:] == SENT).all() and (sx[nb:] == SENT).all(), what + ": sentinel"
    return limbs, u, sx


def _ssq_held(want):
    """blocks whose sum of squares fp32 holds as a normal number (tests/test_gpu_xq_gemv_kernel.py `_check_ssq`)"""
    return (want == 0) | ((want > 2.0 ** -100) & (want < 2.0 ** 100))


def _check_ssq(d_ssq, n, buf32, what):
    s = d_ssq.cpu().numpy()
    assert (s[n // 16:] == SENT).all(), what + ": ssq sentinel"
    want = X.block_ssq(buf32)
    held = _ssq_held(want)
    assert (np.abs(s[:n // 16].astype(np.float64) - want)[held] <= X.SSQ_REL * want[held]).all(), what + ": ssq"
    return s


def _plain(ctx, xs, what, hold=None):
    """one plain all-reduce of the ranks' vectors xs: exact, sentinel intact"""
    n = xs[0].size
    want = T.rank_ordered_sum(xs)
    buf = torch.full((n + 16,), SENT, device="cuda")
    buf[:n] = _dev(xs[ctx.rank])
    if hold == ctx.rank:  # this rank shows up late: the others wait inside the kernel
        torch.cuda._sleep(200_000_000)
    L.probe_comm_allreduce(ctx.comm, buf, n)
    got = buf.cpu().numpy()
    assert (got[n:] == SENT).all(), what + ": written past n"
    assert T.same_bits(got[:n], want), "%s: %d elements differ" % (
        what, int((got[:n].view(np.uint32) != want.view(np.uint32)).sum()))
    ctx.done(what, got[:n])


def _xq_inputs(rng, n, world):
    """N(0, 1) with one element times 30, one all-zero block, one block of magnitude 1e-20 (from three blocks on)"""
    xs = [rng.standard_normal(n).astype(F32) for _ in range(world)]
    nb = n // 16
    for x in xs:
        x[n // 3] *= 30
        if nb >= 3:
            x[(nb // 2) * 16:(nb // 2) * 16 + 16] = 0
            x[(nb - 1) * 16:] *= F32(1e-20)
    return xs


def _xq(ctx, xs, norm_w, with_ssq, what, pushed=False, buf=None):
    """one XQ-emitting all-reduce: buf exact, the XQ vector == encode of the kernel's own buf, ssq, sentinels.
    `buf` given: the device buffer already holds this rank's vector (and has been pushed when pushed is set)."""
    n = xs[0].size
    want = T.rank_ordered_sum(xs)
    y_want = want if norm_w is None else (want * norm_w).astype(F32)
    assert np.isfinite(want).all() and np.isfinite(y_want).all(), what  # encode is specified on finite inputs
    if buf is None:
        buf = torch.full((n + 16,), SENT, device="cuda")
        buf[:n] = _dev(xs[ctx.rank])
    xo = _xo_buffers(n)
    d_ssq = torch.full((n // 16 + 4,), SENT, device="cuda") if with_ssq else None
    L.probe_comm_allreduce(ctx.comm, buf, n, pushed=pushed, norm_w=_dev(norm_w), xo=xo, ssq_out=d_ssq)
    got = buf.cpu().numpy()
    assert (got[n:] == SENT).all(), what + ": written past n"
    assert T.same_bits(got[:n], want), what + ": sum"
    parts = _check_xo(xo, n, got[:n] if norm_w is None else (got[:n] * norm_w).astype(F32), what)
    parts += (_check_ssq(d_ssq, n, got[:n], what),) if with_ssq else ()
    ctx.done(what, got[:n], *parts)
    return (got[:n],) + parts


def _greedy(ctx, pmax, pidx, local_vocab, what, pos0=3, status0=0, want_status=None):
    """one greedy pick over the ranks' pairs: token, log[old pos], pos + 1 and the status word"""
    offsets = [r * local_vocab for r in range(ctx.world)]
    want, want_st = T.greedy_pick(pmax, pidx, offsets)
    if want_status is not None:
        assert want_st == want_status, what
    i32 = lambda v, n=1: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    token, pos, log, status = i32(-5), i32(pos0), i32(-7, 16), i32(status0)
    L.probe_comm_greedy(ctx.comm, _dev(pmax[ctx.rank].astype(F32)), _dev(pidx[ctx.rank].astype(np.int32)),
                        offsets[ctx.rank], token, pos, log, status)
    got = (int(token.item()), int(pos.item()), int(status.item()))
    lg = log.cpu().numpy()
    assert got == (want, pos0 + 1, status0 | want_st), (what, got, want, want_st)
    assert lg[pos0] == want and (np.delete(lg, pos0) == -7).all(), (what, lg)
    ctx.done(what, np.array(got), lg)


def _greedy_pairs(rng, n_pairs, world):
    """random pairs the way lm_head_kernel leaves them: pair i = (a value, a local index inside rows 16 i .. 16 i + 15)"""
    pm = [rng.standard_normal(n_pairs).astype(F32) for _ in range(world)]
    pi = [(16 * np.arange(n_pairs) + rng.integers(0, 16, n_pairs)).astype(np.int32) for _ in range(world)]
    return pm, pi


# ---- A. plain all-reduce -------------------------------------------------------------------------------------------------
A_SIZES = [5008, 1, 4096, 15, 16, 4112, 17, 2048, 1025, 255, 256, 1024, 1023]  # either parity: large, small, large


def _family_plain(ctx):
    assert sorted(A_SIZES) == [1, 15, 16, 17, 255, 256, 1023, 1024, 1025, 2048, 4096, 4112, 5008]
    rng = np.random.default_rng(11)
    for n in A_SIZES:
        _plain(ctx, [_random(rng, n) for _ in range(2)], "plain n %d" % n)
    sp = T.specials(2)
    _plain(ctx, sp, "plain specials")
    _plain(ctx, [np.resize(s, 1025) for s in sp], "plain specials tiled to 1025")  # odd period: every lane meets them
    _plain(ctx, [np.resize(s, 1025) for s in sp[::-1]], "plain specials, ranks swapped")
    for hold in (0, 1):
        _plain(ctx, [_random(rng, 4112) for _ in range(2)], "plain n 4112, rank %d late" % hold, hold=hold)


def test_plain_allreduce_world_2(tmp_path):
    _spawn("plain", 2, tmp_path)


# ---- B. XQ-emitting all-reduce ---------------------------------------------------------------------------------------
B_SIZES = [4096, 16, 5008, 256, 4112, 1024, 1040]


def _family_xq(ctx):
    assert sorted(B_SIZES) == [16, 256, 1024, 1040, 4096, 4112, 5008]
    rng = np.random.default_rng(12)
    for n in B_SIZES:
        xs = _xq_inputs(rng, n, 2)
        g = (1 + 0.1 * rng.standard_normal(n)).astype(F32)
        # what a slip would have to get past, from the reference alone: another norm weight (the reversed one, or
        # none) encodes differently, and sums of squares of buf * norm_w miss the bound on block_ssq(buf)
        s = T.rank_ordered_sum(xs)
        enc = lambda y: np.concatenate([p.astype(np.float64).ravel() for p in X.encode(y.astype(F32))])  # noqa: E731
        assert not np.array_equal(enc(s * g), enc(s)) and not np.array_equal(enc(s * g), enc(s * g[::-1]))
        ssq, ssq_g = X.block_ssq(s), X.block_ssq((s * g).astype(F32))
        held = _ssq_held(ssq) & (ssq > 0)
        assert (np.abs(ssq_g - ssq)[held] > 4 * X.SSQ_REL * ssq[held]).any()
        for norm in (False, True):
            for with_ssq in (False, True):
                _xq(ctx, xs, g if norm else None, with_ssq,
                    "xq n %d%s%s" % (n, " norm" if norm else "", " ssq" if with_ssq else ""))


def test_xq_emitting_allreduce_world_2(tmp_path):
    _spawn("xq", 2, tmp_path)


# ---- C. pushed form ------------------------------------------------------------------------------------------------------
C_GEOMETRY = {128: [(1, 1, 4)], 2048: [(16, 4, 4)], 4096: [(32, 4, 8)], 14336: [(112, 14, 8)],
              16512: [(65, 9, 8), (64, 8, 8)]}
C_CASES = [(K, N) for K in (128, 2048, 4096) for N in (256, 4096)] + [(14336, 32), (16512, 32), (2048, 40)]


def _shard(K, N, form, rank, seed):
    """rank's row-parallel shard [K, N] of a projection, RTN-quantised by the oracle -> (q, s, z)"""
    from oracle import woq_oracle as orc

    rng = np.random.default_rng([seed, rank])
    w = (0.05 * rng.standard_normal((N, K), dtype=np.float32))
    return orc.rtn_quantize(w, True, form[0], form[1])


def _shard_blob(q, s, z, form):
    from intel_extension_for_transformers_amd import qbits

    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    return qbits.repack_quantized_weight(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(),
                                         e8 if z is None else torch.from_numpy(z).cuda(), e32, "int4_clip", form[2],
                                         "fp32", form[1], form[0])


def _pushed_case(ctx, K, N, form, seed):
    what = "pushed K %d N %d g%d" % (K, N, form[0])
    smode = 1 if form[0] < 128 else 0
    geom = [(c, nw, tpw) for _, c, nw, tpw, _ in X.geometry(K, 0, smode, 0)]
    assert geom == C_GEOMETRY[K], (what, geom)
    rng = np.random.default_rng([seed, 99])
    npad = (N + 15) // 16 * 16
    xs = [rng.standard_normal(K).astype(F32) for _ in range(2)]
    for x in xs:
        x[K // 3] *= 30
    residual = rng.standard_normal(N).astype(F32)  # rank 0 alone adds it (the engine's tp_residual)
    g_next = (1 + 0.1 * rng.standard_normal(npad)).astype(F32)
    blobs = [_shard_blob(*_shard(K, N, form, r, seed), form) for r in range(2)]
    # both ranks' shards through the plain probe: the partial sums every rank expects
    plain = []
    for r in range(2):
        o = torch.full((npad + 16,), SENT, device="cuda")
        L.probe_gemv_xq(_dev(xs[r]), blobs[r], 0, residual=_dev(residual) if r == 0 else None, out=o)
        plain.append(o.cpu().numpy())
        assert (plain[r][N:] == SENT).all() and np.isfinite(plain[r][:N]).all(), what
    # this rank's shard through the pushing probe: the same `out`
    buf = torch.full((npad + 16,), SENT, device="cuda")
    buf[N:npad] = 0  # ragged N: the dead columns of the residual stream are 0 on every rank
    L.probe_gemv_xq_tp(ctx.comm, _dev(xs[ctx.rank]), blobs[ctx.rank], 0,
                       residual=_dev(residual) if ctx.rank == 0 else None, out=buf)
    mine = buf.cpu().numpy()
    assert np.array_equal(mine[:N].view(np.uint32), plain[ctx.rank][:N].view(np.uint32)), what + ": out differs"
    assert (mine[N:npad] == 0).all() and (mine[npad:] == SENT).all(), what + ": written past N"
    parts = [np.concatenate([p[:N], np.zeros(npad - N, F32)]) for p in plain]
    if N == npad:
        first = _xq(ctx, parts, g_next, True, what + " pushed=1", pushed=True, buf=buf)
    else:
        # nothing is pushed for columns >= N: the pushed all-reduce is the plain variant over the N live columns
        want = T.rank_ordered_sum([p[:N] for p in parts])
        L.probe_comm_allreduce(ctx.comm, buf, N, pushed=True)
        got = buf.cpu().numpy()
        assert T.same_bits(got[:N], want) and (got[N:npad] == 0).all() and (got[npad:] == SENT).all(), what
        ctx.done(what + " pushed=1, plain variant", got[:N])
        first = None
    # the same partials without the push: identical bytes
    second = _xq(ctx, parts, g_next, True, what + " pushed=0")
    if first is not None:
        for a, b in zip(first, second):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + ": pushed=1 and pushed=0 differ"
    else:
        assert np.array_equal(second[0][:N].view(np.uint32), got[:N].view(np.uint32)) and (second[0][N:] == 0).all(), what


def _family_pushed(ctx):
    for i, (K, N) in enumerate(C_CASES):
        for j, form in enumerate((G128, G32A)):
            _pushed_case(ctx, K, N, form, 100 + 2 * i + j)


def test_pushed_form_world_2(tmp_path):
    _spawn("pushed", 2, tmp_path)


# ---- D. the wrap of the sequence number, graph replays ---------------------------------------------------------------
def _family_replay(ctx):
    import torch.distributed as dist

    rng = np.random.default_rng(14)
    g = (1 + 0.1 * rng.standard_normal(4096)).astype(F32)
    local_vocab = 24 * 16
    # the wrap first, while the inbox holds no tag yet (woq_probe_comm_set_seq): 0xfffffffd, 0xfffffffe, 0xffffffff, 2, 3, 4
    torch.cuda.synchronize()
    dist.barrier()
    L.probe_comm_set_seq(ctx.comm, 0xFFFFFFFD)
    for i in range(2):
        _plain(ctx, [_random(rng, 1025) for _ in range(2)], "wrap %d: plain n 1025" % i)
        _xq(ctx, _xq_inputs(rng, 4096, 2), g, True, "wrap %d: xq n 4096" % i)
        _greedy(ctx, *_greedy_pairs(rng, 24, 2), local_vocab, "wrap %d: greedy" % i)
    with pytest.raises(RuntimeError, match="QBits: 0 is never a live sequence number"):
        L.probe_comm_set_seq(ctx.comm, 0)
    # one graph of three collectives: each of them changes its buffer from one replay to the next
    buf_x = torch.full((4096 + 16,), SENT, device="cuda")
    buf_p = torch.full((1025 + 16,), SENT, device="cuda")
    xo, d_ssq, d_g = _xo_buffers(4096), torch.full((4096 // 16 + 4,), SENT, device="cuda"), _dev(g)
    pmax, pidx = torch.zeros(24, device="cuda"), torch.zeros(24, dtype=torch.int32, device="cuda")
    i32 = lambda v, n=1: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    token, pos, log, status = i32(-5), i32(0), i32(-7, 16), i32(0)

    def chain():
        L.probe_comm_allreduce(ctx.comm, buf_x, 4096, norm_w=d_g, xo=xo, ssq_out=d_ssq)
        L.probe_comm_allreduce(ctx.comm, buf_p, 1025)
        L.probe_comm_greedy(ctx.comm, pmax, pidx, ctx.rank * local_vocab, token, pos, log, status)

    def load():
        xs, ps, (pm, pi) = _xq_inputs(rng, 4096, 2), [_random(rng, 1025) for _ in range(2)], _greedy_pairs(rng, 24, 2)
        buf_x[:4096] = _dev(xs[ctx.rank])
        buf_p[:1025] = _dev(ps[ctx.rank])
        pmax.copy_(_dev(pm[ctx.rank]))
        pidx.copy_(_dev(pi[ctx.rank]))
        return xs, ps, pm, pi

    def check(what, loaded, step):
        xs, ps, pm, pi = loaded
        torch.cuda.synchronize()
        bx, bp = buf_x.cpu().numpy(), buf_p.cpu().numpy()
        assert (bx[4096:] == SENT).all() and (bp[1025:] == SENT).all(), what
        assert T.same_bits(bx[:4096], T.rank_ordered_sum(xs)) and T.same_bits(bp[:1025], T.rank_ordered_sum(ps)), what
        parts = _check_xo(xo, 4096, (bx[:4096] * g).astype(F32), what)
        s = _check_ssq(d_ssq, 4096, bx[:4096], what)
        want, want_st = T.greedy_pick(pm, pi, [0, local_vocab])
        lg = log.cpu().numpy()
        assert want_st == 0 and (int(token.item()), int(pos.item()), int(status.item())) == (want, step + 1, 0), what
        assert lg[step] == want and (lg[step + 1:] == -7).all(), what
        ctx.done(what, bx[:4096], bp[:1025], s, lg, *parts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # once eagerly on the capture stream: nothing is loaded or allocated under capture
        loaded = load()
        chain()
        check("eager chain before the capture", loaded, 0)
    loaded = load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain()
    for rep in range(4):
        if rep:
            loaded = load()
        graph.replay()
        check("replay %d" % rep, loaded, 1 + rep)


def test_sequence_wrap_and_graph_replays_world_2(tmp_path):
    _spawn("replay", 2, tmp_path)


# ---- E. greedy pick ------------------------------------------------------------------------------------------------------
def _greedy_cases(ctx, n_pairs_list):
    rng = np.random.default_rng(15)
    W, s = ctx.world, T.SENTINEL
    for n_pairs in n_pairs_list:
        lv = n_pairs * 16
        last = n_pairs - 1
        for r in (0, W - 1):  # the winner on the first and on the last rank, in the last pair (beyond 1024 threads at 2000)
            pm, pi = _greedy_pairs(rng, n_pairs, W)
            pm[r][last] = 9.0
            _greedy(ctx, pm, pi, lv, "greedy %d pairs: winner on rank %d" % (n_pairs, r), pos0=r)
        pm, pi = _greedy_pairs(rng, n_pairs, W)  # equal maxima on every rank: the lowest global index, rank 0's
        for r in range(W):
            pm[r][(last * (r + 1)) // W] = 9.0
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: equal maxima on all ranks" % n_pairs)
        if n_pairs > 1:  # equal maxima inside the last rank, the lower index listed later; pairs in any order
            pm, pi = _greedy_pairs(rng, n_pairs, W)
            perm = rng.permutation(n_pairs)
            pm[W - 1][[0, last, n_pairs // 2]] = 9.0
            pm[W - 1], pi[W - 1] = pm[W - 1][perm[::-1]], pi[W - 1][perm[::-1]]
            _greedy(ctx, pm, pi, lv, "greedy %d pairs: equal maxima inside a rank" % n_pairs)
        pm, pi = _greedy_pairs(rng, n_pairs, W)  # rank 0 has nothing to offer
        pm[0][:], pi[0][:] = -np.inf, s
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: rank 0 all -inf under the sentinel" % n_pairs)
        pm, pi = _greedy_pairs(rng, n_pairs, W)
        pm[W - 1][:] = np.nan
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: last rank all NaN" % n_pairs)
        pm, pi = _greedy_pairs(rng, n_pairs, W)  # -inf under a real index is a candidate, and beats the sentinel
        for r in range(W):
            pm[r][:] = -np.inf
            pi[r][:last] = s
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: -inf everywhere, one real index a rank" % n_pairs, want_status=0)
        # no winner anywhere: token 0 and status bit 2 (kept beside an earlier bit), on every rank
        pm, pi = _greedy_pairs(rng, n_pairs, W)
        for r in range(W):
            pm[r][:] = np.nan
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: every pair NaN" % n_pairs, want_status=4)
        for r in range(W):
            pm[r][:], pi[r][:] = -np.inf, s
        _greedy(ctx, pm, pi, lv, "greedy %d pairs: every pair -inf under the sentinel" % n_pairs, status0=2, want_status=4)


def _family_greedy(ctx):
    _greedy_cases(ctx, [24, 1, 2000])


def test_greedy_pick_world_2(tmp_path):
    _spawn("greedy", 2, tmp_path)


# ---- F. world 4 ----------------------------------------------------------------------------------------------------------
def _family_world4(ctx):
    rng = np.random.default_rng(16)
    for n in (1025, 17, 4096):
        xs = [_random(rng, n) for _ in range(4)]
        # four addends: the order decides the bits, so a kernel that summed in another order is caught on these inputs
        # (49 and 207 elements of the two long vectors; magnitudes 2^120 apart leave none among 17 elements)
        assert n == 17 or not np.array_equal(T.rank_ordered_sum(xs), T.rank_ordered_sum(xs[::-1])), n
        _plain(ctx, xs, "world 4 plain n %d" % n)
    _plain(ctx, T.specials(4), "world 4 specials")
    _greedy_cases(ctx, [24])


def test_plain_allreduce_and_greedy_pick_world_4(tmp_path):
    _spawn("world4", 4, tmp_path)


FAMILIES = {"plain": _family_plain, "xq": _family_xq, "pushed": _family_pushed, "replay": _family_replay,
            "greedy": _family_greedy, "world4": _family_world4}
