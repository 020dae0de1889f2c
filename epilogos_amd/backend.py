"""Compute backend used by the stage drivers (expected.py / scores.py / driver.py).

There is exactly one product backend: HipBackend (the gfx950 kernels through the C ABI).  It raises when the HIP
library or a GPU is missing -- there is no CPU fallback.  `set_for_testing` exists so that the CPU-only test-suite
can exercise the host logic (file naming, partitioning, the gloo collective path) with an oracle-backed stand-in;
nothing in the package ever installs one.
"""
import collections
import os

import numpy as np

_override = None


class HipBackend:
    """Host-array facade over epilogos_amd.engine (device tensors inside)."""
    name = "hip"

    def __init__(self, device=None):
        import torch
        from . import engine
        engine.require_gpu()
        self.torch = torch
        self.engine = engine
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device

    # ---- transfers
    def to_device(self, x):
        return self.engine.states_to_device(x, device=self.device)

    # ---- expected pass (STEP 1): integer counts as host arrays with the reference's dtypes/shapes
    def expected_counts(self, x, S, saliency):
        eng = self.engine
        N = x.shape[1]
        X = self.to_device(x)
        if saliency == 1:
            _, c = eng.bin_hist(X, N, S, want_hist=False)
            return c.cpu().numpy()
        if saliency == 2:
            _H, c2 = eng.bin_hist_s2(X, N, S)
            return c2.cpu().numpy().reshape(S, S)
        if saliency == 3:
            return eng.hist_s3(X, N, S).cpu().numpy().reshape(N, N, S, S)
        raise ValueError("Please ensure that saliency metric is either 1, 2, or 3")

    def check_counts(self, counts, R, N, saliency):
        """Every state byte must have been counted: a byte outside [0, S) is silently skipped by the kernels.  `counts` is
        the count array or its already computed total."""
        total = int(counts) if np.ndim(counts) == 0 else int(np.asarray(counts, dtype=np.int64).sum())
        want = R * N if saliency == 1 else R * N * (N - 1)
        if total != want:
            raise ValueError("input contains states outside 1..numStates (counted %d of %d)" % (total, want))

    # ---- combination (STEP 2)
    def normalise(self, counts):
        t = self.torch.from_numpy(np.ascontiguousarray(counts).reshape(-1)).to(self.device)
        return self.engine.normalise(t).cpu().numpy().reshape(np.shape(counts))

    # ---- score pass (STEP 3): float32 [R, S] exactly as the reference stores it
    def scores(self, x, S, saliency, q, perms=None):
        eng = self.engine
        N = x.shape[1]
        X = self.to_device(x)
        qd = q.reshape(-1) if self.torch.is_tensor(q) else \
            self.torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32).reshape(-1)).to(self.device)
        if saliency == 1:
            o32 = self._score_s1_host_table(eng.bin_hist(X, N, S, want_counts=False)[0], N, S, q)
        elif saliency == 2:
            o32, _ = eng.score_s2(X, N, S, qd, perms=perms)
        elif saliency == 3:
            o32, _ = eng.score_s3(X, N, S, qd)
        else:
            raise ValueError("Please ensure that saliency metric is either 1, 2, or 3")
        return o32.cpu().numpy()

    def _score_s1_host_table(self, H, N, S, q):
        """S1 scores from histograms through the table the host builds with the reference's arithmetic (scores.s1ScoreTable):
        float32 values identical to the reference's, hence identical text."""
        from .scores import s1ScoreTable
        qh = q.cpu().numpy() if self.torch.is_tensor(q) else np.asarray(q, dtype=np.float32)
        _t64, t32 = s1ScoreTable(qh.reshape(-1), N)
        o32, _ = self.engine.score_s1_from_binhist_table(H, N, S, T32=self.torch.from_numpy(t32).to(self.device))
        return o32

    # ---- paired extras
    def pair_finish(self, a, b):
        ta = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        tb = self.torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(self.device)
        d, dist = self.engine.pair_finish(ta, tb)
        return d.cpu().numpy(), dist.cpu().numpy()

    def pair_metrics(self, delta, roundtrip=True):
        td = self.torch.from_numpy(np.ascontiguousarray(delta, dtype=np.float32)).to(self.device)
        dist, maxdiff = self.engine.pair_metrics(td, roundtrip)
        return dist.cpu().numpy(), maxdiff.cpu().numpy()

    def quiescent(self, xa, xb, qstate):
        m = self.engine.quiescent(self.to_device(xa), xa.shape[1], self.to_device(xb), xb.shape[1], qstate)
        return m.cpu().numpy().astype(bool)

    def null_scores(self, xa, xb, S, saliency, q, groupSize, seed, row0=0):
        """Scores of the two shuffled null halves (reference helpers.py:183-194 + scores.py:321-322,418-421)."""
        eng = self.engine
        NA, NB = xa.shape[1], xb.shape[1]
        ga, gb = _null_widths(NA, NB, groupSize)
        if S > 31:                                       # the wide models: the matrix-scanning kernel decodes five bits
            hA, _ = eng.bin_hist(self.to_device(xa), NA, S, want_counts=False)
            hB, _ = eng.bin_hist(self.to_device(xb), NB, S, want_counts=False)
            HA, HB = eng.null_hist_from_binhist(hA, hB, NA + NB, S, ga, gb, seed, row0)
        else:
            HA, HB = eng.null_hist(self.to_device(xa), NA, self.to_device(xb), NB, S, ga, gb, seed, row0)
        qd = self.torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32).reshape(-1)).to(self.device)
        if saliency == 1:
            na, nb = self._score_s1_host_table(HA, ga, S, q), self._score_s1_host_table(HB, gb, S, q)
        elif saliency == 2:
            # quirk Q9: the null halves keep the ORIGINAL groups' permutation counts (scores.py:397-398,418-421)
            na, _ = eng.score_s2_from_binhist(HA, max(ga, NA), S, qd, perms=NA * (NA - 1))
            nb, _ = eng.score_s2_from_binhist(HB, max(gb, NB), S, qd, perms=NB * (NB - 1))
        else:
            raise ValueError("Please ensure that saliency metric is either 1 or 2 for Pairwise Epilogos")
        return na.cpu().numpy(), nb.cpu().numpy()


    # ---- device-resident sessions of the genome-wide driver (driver.py): every part is uploaded ONCE, its per-bin
    # histograms (S1/S2) or its state matrix (S3, paired) stay in HBM between the count pass and the score pass
    def open_single(self, S, saliency):
        return _HipSingleSession(self, S, saliency)

    def open_paired(self, S, saliency, quiescentState, groupSize, seed, draws=1):
        return _HipPairedSession(self, S, saliency, quiescentState, groupSize, seed, draws)


def _null_widths(NA, NB, groupSize):
    """Widths of the two null groups: the real groups' by default, `groupSize` each with -g."""
    return (NA, NB) if groupSize == -1 else (groupSize, groupSize)


def _count_shape(saliency, S, N):
    """Shape of the count array (and of exp_freq) of a saliency level."""
    return {1: (S,), 2: (S, S), 3: (N, N, S, S)}[saliency]


def _unless_unsupported(fn, *args, **kw):
    """fn(*args, **kw), or None when the kernel does not take these shapes (EPG_ERR_UNSUPPORTED); the caller then takes the
    separate launches that give the same results."""
    from ._abi import EpilogosHipError
    try:
        return fn(*args, **kw)
    except EpilogosHipError as e:
        if e.code != -2:
            raise
        return None


def _aligned_rows(T, lo, hi):
    """Rows [lo, hi) of a resident part as the kernels want them: the score entry points take 16-byte aligned bases
    (epg_s1.hip check_score_from_hist_args, epg_null.hip, epg_s2.hip), and a row slice of an [R, S] uint16 array starts at
    lo * S * 2 bytes -- a view only when that is a multiple of 16, else a copy of just these rows."""
    from . import engine
    t = T[lo:hi]
    if engine.aligned16(t) and t.untyped_storage().nbytes() <= 4 * max(t.numel() * t.element_size(), 1):
        return t
    # a copy of just these rows: a misaligned slice -- or one that would keep alive an allocation several times its size (the
    # histograms of a whole batch of parts come from ONE allocation, engine.hist_rows_alloc: a rank that hands most of a batch
    # over to its neighbours and drops it must not keep all of it for the few rows it scores itself)
    return t.clone()


class _HipSession:
    """Shared plumbing: pinned staging, one asynchronous upload per matrix, the count accumulator, the queue of parts that wait
    for their count pass and the early results of the score pass."""

    # parts are COUNTED IN BATCHES: one launch per BATCH_ROWS rows or BATCH_PARTS parts, or when anything needs their histograms
    # (_flush).  A subclass says how a batch is counted (_count) and which parts join the queue.
    BATCH_ROWS, BATCH_PARTS = 8_000_000, 32

    def __init__(self, be, S, saliency):
        self.be, self.S, self.sal = be, S, saliency
        self.torch, self.eng, self.device = be.torch, be.engine, be.device
        self._pool = None                                # page-locked staging (lazily: a session fed device-resident parts has none)
        self._copy_stream = None
        self.held = {}                                   # ticket -> pinned buffer handed to the parser
        self.acc = None
        self.q = None
        self.parts = []
        self.n_uploads = 0
        self.upload_bytes = 0
        self._releaser = None
        self._t1 = {}                                    # S1 score tables (device, float32) by group width
        self._t1_verified = set()
        self.tables_patched = 0
        self._pending_check = None
        self._pending, self._pending_rows = [], 0        # queued parts (what _count needs of each) and their rows
        self._launched = False                           # launch() ran: STEP 2 is on the device, STEP 3 of `_early` parts enqueued
        self._early = {}                                 # part id -> its device results, computed before the host-side checks
        # --check-states: every uploaded matrix is censused where it first sits on the device (_upload); ticket -> (other [N],
        # first_bad [1], the byte at first_bad [1]), device tensors, read by state_offenders()
        self.check_states = False
        self.state_checks = {}
        self._census_scratch = {}

    @property
    def pool(self):
        """Staging buffers in flight; paired mode holds a part's A and B at once, so never fewer than two (first come, first
        served: the driver takes the parts as their parsers finish).  A reader holds its buffer from the moment it knows its
        file's shape until the upload is over -- the parse runs straight into it -- so fewer buffers than readers serialise the
        parse stage (profiles/r04k: four buffers for sixteen readers, every reader waited 0.3-1.7 s).  Half as many as this rank
        may run parser threads, at most 8 (~1 GB of page-locked memory each for a whole-genome run)."""
        if self._pool is None:
            from . import _io
            n = int(os.environ.get("EPILOGOS_PINNED_BUFFERS", min(8, max(4, _io.host_budget() // 2))))
            self._pool = self.be.engine.PinnedPool(max(2, n), in_order=False)
        return self._pool

    @property
    def copy_stream(self):
        if self._copy_stream is None:
            self._copy_stream = self.torch.cuda.Stream(device=self.device)
        return self._copy_stream

    def alloc(self, ticket):
        """-> alloc(R, N) for _io.read_table / helpers.readTable: a pinned, row-padded destination for part `ticket`."""
        def make(R, N):
            ldx = self.eng.padded_width(N)
            buf = self.held.get(ticket)                  # asked twice for one part (helpers.readTable's pandas re-read of a file
            if buf is None or buf.numel() < R * ldx:     # the native parser refused): the same buffer when it fits
                if buf is not None:
                    self.pool.release(self.held.pop(ticket))
                buf = self.pool.acquire(ticket, R * ldx)
                self.held[ticket] = buf
            return buf[:R * ldx].view(R, ldx).numpy()
        return make

    def skip(self, ticket):
        if ticket not in self.held:
            self.pool.skip(ticket)

    def _upload(self, arr, N, ticket):
        """One H2D copy of the staged matrix (pinned -> HBM on the copy stream).  The device buffer is allocated ON the copy
        stream, so the copy waits for nothing the compute stream is doing (round 2 made it wait for the previous part's
        kernels and then blocked the host until the copy was over); the compute stream waits for the copy's event, and the
        staging buffer goes back to the pool from a helper thread once that event has completed."""
        R = arr.shape[0]
        buf = self.held.pop(ticket, None)
        if buf is None:                                  # not staged through alloc(): pageable fallback of the same layout
            self.pool.skip(ticket)
            X = self.eng.states_to_device(arr[:, :N], device=self.device)
        else:
            X, ev = self.eng.upload_states(buf, R, arr.shape[1], self.copy_stream, device=self.device)
            self.torch.cuda.current_stream().wait_event(ev)
            self._release_later(ev, buf)
        self.n_uploads += 1
        self.upload_bytes += X.numel()
        if self.check_states and R and N:
            self._check_upload(X, N, ticket)
        return X

    def stage(self, arr, N, ticket):
        """A parsed matrix -> HBM, the one upload of it (paired mode: one group's matrix of a part, as soon as it is parsed -- its
        staging buffer goes back to the pool at once: a part must not sit on two of the few buffers while its other half is
        still being inflated).  The result feeds add_device / add_staged / add_columns, of this session or -- it is read, never
        written -- of later ones (driver.run_groupings keeps it between its groupings)."""
        return self._upload(arr, N, ticket)

    def check_resident(self, X, N, ticket):
        """--check-states for a matrix that reached the device without an upload of this session (driver.run_groupings with
        resident matrices): the census _upload takes, under the ticket the verdict will look it up by."""
        if self.check_states and X.shape[0] and N:
            self._check_upload(X, N, ticket)

    def close(self):
        """Give back what the session holds: its parts (histograms, state rows, null groups), the early results, the count
        accumulator, exp_freq and the S1 tables, the census scratch, the engine's kept membership bytes of its column groups, and
        the page-locked staging buffers with the thread that returns them.  The matrices a caller passed to add_device / add_columns are the caller's.  A closed session takes no
        further calls."""
        self._pending, self._pending_rows = [], 0
        self.parts, self._early, self._t1, self._t1_verified = [], {}, {}, set()
        self.acc = self.q = self._pending_check = None
        self.state_checks, self._census_scratch = {}, {}
        self.eng.forget_group_members()                  # (the membership bytes of this session's column groups)
        if self._releaser is not None:                   # (waits for the uploads in flight: their staging buffers come back)
            self._release_q.put(None)
            self._releaser.join()
            self._releaser = None
        self.held = {}
        if self._pool is not None:
            self._pool.close()
            self._pool = None

    def _check_upload(self, X, N, ticket):
        """--check-states: the census of a matrix just uploaded, all N columns of it.  The per-state counts go to a scratch table
        nobody reads (the ABI wants one); `other`, `first_bad` and the offending byte itself -- fetched now, the matrix may be
        gone when the verdict is taken -- stay on the device, nothing synchronises."""
        t, eng = self.torch, self.eng
        scratch = self._census_scratch.get(N)
        if scratch is None:
            scratch = self._census_scratch[N] = t.zeros((N, self.S), dtype=t.int64, device=self.device)
        _c, other, fb = eng.state_census(X, N, self.S, census=scratch)
        at = t.where(fb == eng.FIRST_BAD_NONE, t.zeros_like(fb), fb)
        self.state_checks[ticket] = (other, fb, X[at // N, at % N])

    def state_offenders(self):
        """{ticket: (row, column, byte 0 .. 255, how many bytes)} of the uploaded matrices that hold a byte that is no state
        (row and column 0-based, of the first such byte in row-major order).  Synchronises."""
        out = {}
        for ticket, (other, fb, byte) in self.state_checks.items():
            n = int(other.sum().item())
            if n:
                N = other.numel()
                at = int(fb.item())
                out[ticket] = (at // N, at % N, int(byte.item()) & 0xff, n)
        self.state_checks = {}
        self._census_scratch = {}
        return out

    def _release_later(self, ev, buf):
        import queue
        import threading
        if self._releaser is None:
            self._release_q = queue.SimpleQueue()

            def work():
                while True:
                    item = self._release_q.get()
                    if item is None:
                        return
                    e, b = item
                    e.synchronize()                      # (releases the GIL) the copy out of this staging buffer is over
                    self.pool.release(b)
            self._releaser = threading.Thread(target=work, name="epilogos-staging-release", daemon=True)
            self._releaser.start()
        self._release_q.put((ev, buf))

    def _acc(self, N=None):
        """The count accumulator (flat): int64 for S1 / S2, int32 for S3."""
        if self.acc is None:
            t = self.torch
            self.acc = t.zeros(int(np.prod(_count_shape(self.sal, self.S, N))), dtype=t.int32 if self.sal == 3 else t.int64,
                               device=self.device)
        return self.acc

    def _queue(self, item, rows):
        """A part joins the queue of the next count launch; the batch is counted once it is full."""
        self._pending.append(item)
        self._pending_rows += rows
        if self._pending_rows >= self.BATCH_ROWS or len(self._pending) >= self.BATCH_PARTS:
            self._flush()

    def _flush(self):
        """Count the queued parts.  They leave the queue only once their count launch has been issued: a launch that raises
        leaves the queue as it was."""
        if self._pending:
            self._count(self._pending)
            self._pending, self._pending_rows = [], 0

    downloaded = collections.Counter()   # name -> score arrays copied to the host by any session of this process (the writer tests count them)

    def device_text(self, locations, scores):
        """--writer gpu: the BGZF bytes (host uint8 array, no end-of-file block) of the score file of device scores [R, S] with
        `locations`, or None when the device refused a value (engine.scores_text_bgzf)."""
        got = self.eng.scores_text_bgzf(locations, scores)
        return None if got is None else got[0][:got[1]].cpu().numpy()

    def release_text(self):
        """--writer gpu, after the last part: the writer's reusable text, workspace and output buffers go back."""
        self.eng.release_text_buffers()

    def drop_part(self, pid):
        self._flush()
        self.parts[pid] = None

    def ensure_acc(self, N):
        self._flush()                                    # a rank without bins still takes part in the all-reduce
        self._acc(N)

    def all_reduce(self, d):
        self._flush()
        d.all_reduce_tensor(self.acc)                    # RCCL over xGMI: the tensor never leaves HBM

    def _score_s1(self, H, N):
        """S1 score pass: gathers from the [N + 1, S] float32 table of this group width (see _s1_table)."""
        o32, _ = self.eng.score_s1_from_binhist_table(H, N, self.S, T32=self._s1_table(N))
        return o32

    def _s1_table(self, N):
        """The S1 score table of group width N.  finish_device builds the tables of the session's widths ON THE DEVICE in the
        launch that normalises (k_s1_combine; no host round trip between the all-reduce and the score pass); the host-facing
        finish() then compares them bit for bit with the table numpy builds from the same exp_freq by the reference's own
        expression (scores.s1ScoreTable) and replaces a table that differs -- so scores_*.txt.gz stay the reference's bytes
        whatever the last bit of a device logarithm does.  A width nobody announced is built from the host table."""
        if N not in self._t1:
            from .scores import s1ScoreTable
            _t64, t32 = s1ScoreTable(self.q.cpu().numpy(), N)
            self._t1[N] = self.torch.from_numpy(t32).to(self.device)
        return self._t1[N]

    def verify_tables(self):
        """-> number of device-built S1 tables that had to be replaced by the host's (0 = the device's float32 tables ARE the
        reference's).  Synchronises; called by finish()."""
        if self.sal != 1 or self.q is None:
            return 0
        from .scores import s1ScoreTable
        qh = self.q.cpu().numpy()
        patched = 0
        for N, Td in list(self._t1.items()):
            if N in self._t1_verified:
                continue
            _t64, t32 = s1ScoreTable(qh, N)
            if not np.array_equal(Td.cpu().numpy().view(np.uint32).reshape(-1), t32.view(np.uint32).reshape(-1)):
                self._t1[N] = self.torch.from_numpy(t32).to(self.device)
                patched += 1
            self._t1_verified.add(N)
        self.tables_patched += patched
        return patched

    def finish_device(self, total_rows, N):
        """STEP 2 on the device, no host synchronisation: exp_freq (flat device tensor) and, for S1, the score tables.  The
        count check (the reference dies on a state outside the model, expected.py:113; here such a byte is counted nowhere, so
        the total comes out short) is DEFERRED to check(), which whoever takes results off the device calls -- finish(),
        scores(), results() do; S3's 899 MB array is summed at once."""
        self._flush()
        self._pending_check = (self.acc, total_rows, N)
        if self.sal == 3:
            self.check()
            self.q = self.eng.normalise(self.acc)
        elif self.sal == 1:
            widths = [w for w in self._s1_widths() if w] or [N]
            self.q = None
            for w in dict.fromkeys(widths):
                self.q, _T64, T32 = self.eng.s1_tables(self.acc, w, self.S, q=self.q)
                self._t1[w] = T32
        else:
            self.q = self.eng.normalise(self.acc)
        self.acc = None
        return self.q

    def check(self):
        if self._pending_check is not None:
            acc, total_rows, N = self._pending_check
            self._pending_check = None
            self.be.check_counts(int(acc.sum(dtype=self.torch.int64).item()), total_rows, N, self.sal)

    def launch(self, total_rows, N, pids):
        """Everything of STEP 2 and STEP 3 that needs no host: exp_freq (and the S1 tables) on the device, then the score pass
        of the parts `pids` -- all enqueued, no synchronisation.  finish() follows with the host side (count check, table
        verification, exp_freq as a host array); scores() / results() then hand the parts' results out.  This is the one
        sequence both the command line (driver.run_single / run_paired) and bench.py's step run."""
        self.finish_device(total_rows, N)
        self.launch_scores(pids)

    def launch_scores(self, pids):
        """The second half of launch() (for a caller that wants an event between STEP 2 and STEP 3)."""
        self._launched = True
        self._begin([p for p in pids if p is not None])

    def _settle(self):
        for pid in self._early:                          # verified: the resident data of the scored parts can go
            self.parts[pid] = None

    def finish(self, total_rows, N):
        """The host side of STEP 2: the count check (the reference dies on a state outside the model, expected.py:113), the
        device-built S1 tables against numpy's (a table that differs is replaced and the parts scored before are scored
        again: never seen, tools/s1_table_probe.py), exp_freq as the host array that is saved."""
        if not self._launched:
            self.finish_device(total_rows, N)
        self._launched = False
        self.check()
        if self.verify_tables() and self._early:
            self._begin(list(self._early))               # (the early results came from a table that was replaced)
        self._settle()
        return self.q.cpu().numpy().reshape(_count_shape(self.sal, self.S, N))


class _Batch:
    """S1 parts of one group width counted in one launch: their histograms are rows of `flat` (part i from starts[i], rows[i]
    rows), so the batch can be scored in one launch too."""
    __slots__ = ("pids", "flat", "starts", "rows", "N")

    def __init__(self, pids, flat, starts, rows, N):
        self.pids, self.flat, self.starts, self.rows, self.N = pids, flat, starts, rows, N


class _Part:
    """A single-mode part.  D: what its score pass reads -- histograms (S1, S2) or state rows (S3) -- or None while the part waits
    in the count queue.  batch: the _Batch whose flat buffer D is a view of (None: D is an allocation of its own)."""
    __slots__ = ("D", "batch")

    def __init__(self, D=None, batch=None):
        self.D, self.batch = D, batch


class _HipSingleSession(_HipSession):
    def __init__(self, be, S, saliency):
        if saliency not in (1, 2, 3):
            raise ValueError("Please ensure that saliency metric is either 1, 2, or 3")
        super().__init__(be, S, saliency)
        self.N = 0                                       # the widest part's width (an empty file has none)
        self._ws3 = None                                 # S3: ONE workspace for all parts of the session

    def add_part(self, arr, N, ticket, columns=None):
        return self.add_device(self._upload(arr, N, ticket), N, columns=columns)

    # S1 parts of less than a GiB -- the chromosome files of a genome -- are counted in batches (the queue of _HipSession): one
    # epg_bin_hist_parts launch per 8 M rows or 32 parts, histograms in one flat allocation, and later ONE score launch over that
    # allocation.  Per part this was 24 count launches and 24 score launches of 0.1-0.25 ms with their ramps and tails: 3.42 ms
    # per 15 M-bin genome against 2.6 ms as one matrix (bench.py s1_paths, round 6); in batches the same job is two count
    # launches and two score launches.  Same integers, same float32 scores.
    def add_device(self, X, N, place=None, columns=None):
        """Count pass over a RESIDENT part -- the ONE entry of the command line (add_part, after its upload), of bench.py and of
        library callers.  place=None (everybody's default): engine.alloc_hist decides -- the histogram cache of a matrix of a GiB
        or more goes where its search finds another memory class than the matrix's (a process-lifetime home block, one bounded
        probe per device), anything smaller gets a plain allocation, and so does everything when placement is off
        (engine.placement_enabled: EPILOGOS_PLACEMENT=0, ranks sharing a GPU).  The command line's parts are one chromosome file
        each -- under a GiB up to ~880 columns -- so a whole-genome run of the reference's shape counts with plain allocations
        (bench.py reports that figure as placement.unplaced; its count passes hide under the parse anyway) while a caller that holds
        the genome as one matrix gets the placed cache.  place=False forces a plain allocation and a count launch of the part's
        own (bench.py's comparison).  columns (0-based indices into the N columns): the part is that GROUP of the matrix's
        biosamples -- its width everywhere behind the count pass is the group's (_add_columns)."""
        if columns is not None:
            return self._add_columns(X, N, columns, place)
        eng, S = self.eng, self.S
        self.N = max(self.N, N or 0)
        pid = len(self.parts)
        if X.shape[0] == 0 or not N:                     # an empty part: nothing to count, and the ABI rejects a zero width
            self.parts.append(_Part(self.torch.empty((0, S), dtype=self.torch.int16, device=self.device) if self.sal < 3 else X))
        elif self.sal == 1 and place is None and X.numel() < eng.PLACE_MIN_BYTES:
            self.parts.append(_Part())
            self._queue((pid, X, N), X.shape[0])
        elif self.sal == 3:
            eng.hist_s3(X, N, S, counts=self._acc(N), ws=self._s3_workspace(X.shape[0], N))
            self.parts.append(_Part(X))
        else:                                            # (S2: the count pass with the pair counts folded in, one launch)
            H = eng.alloc_hist(X, N, S) if place is not False else None
            H, _ = eng.bin_hist(X, N, S, counts=self._acc(), H=H) if self.sal == 1 else eng.bin_hist_s2(X, N, S, counts2=self._acc(), H=H)
            self.parts.append(_Part(H))
        return pid

    def _add_columns(self, X, N, columns, place):
        """A part that is a column group of a resident matrix.  S1 / S2 of a state model: the grouped count pass reads the whole
        rows once and leaves the histograms of the group's columns (epg_bin_hist_groups); the part then is what a matrix cut
        to these columns would have left.  S3 (its score pass reads the states) and the wide models: the columns are gathered on
        the device and the ordinary path runs on the result."""
        eng, S = self.eng, self.S
        cols = eng.check_columns(columns, N or 0)
        n = int(cols.size)
        if X.shape[0] == 0 or not n or self.sal == 3 or S > eng.GROUPS_MAX_STATES:
            return self.add_device(eng.select_columns(X, cols), n, place=place)
        self.N = max(self.N, n)
        Hs, _ = eng.bin_hist_groups(X, N, S, [cols], counts=self._acc() if self.sal == 1 else None)
        if self.sal == 2:
            eng.hist_s2_from_binhist(Hs[0], S, counts=self._acc())
        self.parts.append(_Part(Hs[0]))
        return len(self.parts) - 1

    def close(self):
        self._ws3 = None
        super().close()

    def _s3_workspace(self, R, N):
        """The ~8 GB workspace of the S3 matrix-core contraction (count pass) and of the S3 score pass (table, transposed matrix,
        cells), grown to the largest part (round 2 allocated and freed one per part: freed device memory is scrubbed at every
        HBM kernel's expense)."""
        need = self.eng.hist_s3_ws_bytes(R, N, self.S)
        if self._ws3 is None or self._ws3.numel() < need:
            self._ws3 = None
            self._ws3 = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
        return self._ws3

    def _count(self, batch):
        """The count pass of queued S1 parts: one launch (per schedule class of their widths), histograms from one allocation."""
        eng, S = self.eng, self.S
        rows = [X.shape[0] for _pid, X, _N in batch]
        flat, starts = eng.hist_rows_flat(rows, S, self.device)
        Hs = [flat[a:a + r] for a, r in zip(starts, rows)]
        eng.bin_hist_parts([X for _pid, X, _N in batch], [N for _pid, _X, N in batch], S, counts=self._acc(), Hs=Hs)
        widths = {N for _pid, _X, N in batch}
        b = _Batch([pid for pid, _X, _N in batch], flat, starts, rows, widths.pop()) if len(widths) == 1 else None
        for (pid, _X, _N), H in zip(batch, Hs):
            self.parts[pid] = _Part(H, b)

    # ---- multi-rank hand-over (driver._redistribute): a part is what the score pass reads -- per-bin histograms (S1, S2)
    # or state rows (S3)
    n_export = 1

    def slice_part(self, pid, lo, hi, row0=None):
        self._flush()
        self.parts.append(_Part(_aligned_rows(self.parts[pid].D, lo, hi)))
        return len(self.parts) - 1

    def export_rows(self, pid, lo, hi):
        self._flush()
        return [self.parts[pid].D[lo:hi]]

    def import_rows(self, tensors, N, row0=None):
        self.N = N
        self.parts.append(_Part(tensors[0].to(self.device)))
        return len(self.parts) - 1

    def ensure_acc(self, N):
        self.N = N
        super().ensure_acc(N)

    def finish(self, total_rows, N):
        self._ws3 = None                                 # (S3: the count pass's workspace goes; the score pass sizes its own)
        return super().finish(total_rows, N)

    def scores_device(self, pid, keep=False):
        """float32 [R, S] scores of part `pid` from its resident data, as a device tensor."""
        self._flush()
        eng, S, N = self.eng, self.S, self.N
        D = self.parts[pid].D
        if not keep:
            self.parts[pid] = None                       # the part's device data is released with its scores
        if D.shape[0] == 0:
            return self.torch.empty((0, S), dtype=self.torch.float32, device=self.device)
        if self.sal == 1:
            return self._score_s1(D, N)
        if self.sal == 2:
            return eng.score_s2_from_binhist(D, N, S, self.q)[0]
        return eng.score_s3(D, N, S, self.q, ws=self._s3_workspace(D.shape[0], N))[0]

    def _s1_widths(self):
        return [self.N]

    def _begin(self, pids):
        self._flush()
        want = [pid for pid in pids if self.parts[pid] is not None]
        asked = set(want)
        self._early = {}
        # a batch whose parts are all asked for and still hold the rows its count pass left: ONE score launch over its flat
        # histogram buffer, the parts' scores are views of one flat result (the <= 7 rows between two parts are scored too)
        batches = {self.parts[pid].batch for pid in want} - {None}
        for b in sorted(batches, key=lambda b: b.pids[0]):                # (in the order they were counted)
            if b.N == self.N and all(pid in asked and self.parts[pid].batch is b for pid in b.pids):
                o32 = self._score_s1(b.flat, self.N)
                for pid, a, r in zip(b.pids, b.starts, b.rows):
                    self._early[pid] = o32[a:a + r]
        for pid in want:
            if pid not in self._early:
                self._early[pid] = self.scores_device(pid, keep=True)

    def early_scores(self, pid):
        """Device tensor of a part scored by launch() (bench.py: the scores stay in HBM)."""
        return self._early[pid]

    def scores(self, pid, text=None):
        """Host array of part `pid`'s scores.  text (the part's _io.Locations; --writer gpu): -> (the array, its score file's BGZF
        bytes from the device or None when the device refused a value) -- the array still comes down, STEP 4 reads it."""
        self.check()
        if pid in self._early:
            self.parts[pid] = None
            dev = self._early.pop(pid)
        else:
            dev = self.scores_device(pid)
        self.downloaded["scores"] += 1
        if text is None:
            return dev.cpu().numpy()
        return dev.cpu().numpy(), self.device_text(text, dev)


class _Pair:
    """A paired-mode part: the two groups' state rows (XA, XB; None for rows taken over from another part or rank), their
    histograms (HA, HB; None while the part waits in the count queue), the shuffle key of its first row (row0), its null
    groups' histograms (HnA, HnB; None until drawn) and the event that says they are (null_done; None: drawn on the main
    stream)."""
    __slots__ = ("XA", "XB", "HA", "HB", "row0", "HnA", "HnB", "null_done")

    def __init__(self, XA, XB, HA, HB, row0, HnA=None, HnB=None):
        self.XA, self.XB, self.HA, self.HB, self.row0 = XA, XB, HA, HB, row0
        self.HnA, self.HnB, self.null_done = HnA, HnB, None


class _HipPairedSession(_HipSession):
    # --null-draws: the buffers of one chunk of draws (null distances, sort keys, sort temporary) stay under this many bytes
    NULL_CHUNK_BYTES = 2 << 30

    def __init__(self, be, S, saliency, quiescentState, groupSize, seed, draws=1):
        if saliency not in (1, 2):
            raise ValueError("Please ensure that saliency metric is either 1 or 2 for Pairwise Epilogos")
        if int(draws) < 1:
            raise ValueError("the number of null draws per bin must be at least 1")
        super().__init__(be, S, saliency)
        self.qstate, self.groupSize, self.seed = quiescentState, groupSize, seed
        # K > 1 null draws per bin (_exceed): the results carry "exceed", null_pool is the size of the pooled null
        self.draws = int(draws)
        self.null_chunk_bytes = self.NULL_CHUNK_BYTES
        self.null_chunks = 0                             # chunks the last exceedance pass took
        self.null_fused = None                           # ... and whether the draws kernel took the shape (False: the loop)
        self._null_kept = None                           # device scalar: the non-quiescent bins of that pass
        self.NA = self.NB = 0                            # the widest part's widths (an empty file pair has none)
        # rows per batch: the default group sizes take the fused kernel (nothing to overlap: two launches per genome, 4.62 ms per
        # 15 M bins against 4.71 with seven); the two-kernel path overlaps batch k's sampler with batch k + 1's count pass
        # (1 / 2 / 3 / 4 M rows: 5.04 / 5.05 / 5.12 / 5.10 ms before the score pass prefetched, one batch 6.1)
        self.BATCH_ROWS = 8_000_000 if groupSize == -1 else 2_000_000
        if getattr(be, "_null_stream", None) is None:    # one second stream per backend, not per session (used by the two-kernel path)
            be._null_stream = self.torch.cuda.Stream(device=self.device)
        self.null_stream = be._null_stream

    def add_part(self, arrA, NA, ticketA, arrB, NB, ticketB, row0):
        return self.add_staged(self._upload(arrA, NA, ticketA), NA, self._upload(arrB, NB, ticketB), NB, row0)

    def close(self):
        self._null_kept = None
        super().close()

    # a batch of parts is counted in ONE launch (epg_bin_hist_parts over the A and the B matrices of all its parts) and its null
    # groups are drawn in ONE launch on the second stream, under the count pass of the next batch (the sampler is VALU-bound,
    # the count pass HBM-bound: tools/overlap_probe.py).  Round 4 launched per part: 2 x 24 count passes of ~80 us and 24 samplers
    # for a genome, each with its ramp and tail -- the count phase of BASELINE config 5 ran at 0.36 of its bytes.
    def add_staged(self, XA, NA, XB, NB, row0):
        """One part's two groups, resident.  row0 keys the null shuffle of the part's first row: the driver passes
        (file ordinal << 40) + row in the file -- known the moment a file is parsed, whatever the partition.  The part joins
        the count queue; the batch is launched when it holds BATCH_ROWS rows (half a genome with the fused kernel, an eighth
        with the two-kernel path: a streaming run still counts while it parses) or 32 parts, or when anything needs its
        histograms."""
        self.NA, self.NB = max(self.NA, NA or 0), max(self.NB, NB or 0)
        pid = len(self.parts)
        if XA.shape[0] == 0 or not NA or not NB:         # nothing to count (and the ABI rejects a zero width)
            t = self.torch
            self.parts.append(_Pair(XA, XB, t.empty((0, self.S), dtype=t.int16, device=self.device),
                                    t.empty((0, self.S), dtype=t.int16, device=self.device), row0))
            return pid
        self.parts.append(_Pair(XA, XB, None, None, row0))
        self._queue((pid, NA, NB), XA.shape[0])
        return pid

    def add_columns(self, X, N, colsA, colsB, row0):
        """One part whose two groups are column groups (0-based indices) of ONE resident matrix: a single grouped launch reads
        the rows once and leaves both groups' histograms; the null groups are drawn from them (the same draws as from the
        matrices: they depend on the histograms, the seed and row0 only).  Wide models gather the two groups and go on as
        add_staged."""
        eng, S = self.eng, self.S
        a, b = eng.check_columns(colsA, N or 0), eng.check_columns(colsB, N or 0)
        NA, NB = int(a.size), int(b.size)
        if np.intersect1d(a, b).size:                    # (no cut-file run has a biosample in both groups)
            raise ValueError("column %d is in both groups" % int(np.intersect1d(a, b)[0]))
        if X.shape[0] == 0 or not NA or not NB or S > eng.GROUPS_MAX_STATES:
            return self.add_staged(eng.select_columns(X, a), NA, eng.select_columns(X, b), NB, row0)
        self.NA, self.NB = max(self.NA, NA), max(self.NB, NB)
        (HA, HB), counts = eng.bin_hist_groups(X, N, S, [a, b])
        if self.sal == 1:
            self._acc().add_(counts[0] + counts[1])     # counts over [A|B] = counts of A + counts of B (helpers.py:173)
        else:
            eng.hist_s2_from_binhist_pair(HA, HB, S, counts=self._acc())
        p = _Pair(None, None, HA, HB, row0)
        self.parts.append(p)
        self._start_null([p])
        return len(self.parts) - 1

    def _count(self, batch):
        """Count pass of a batch and its null groups.  The default group sizes, a state model and widths the fused kernel takes:
        ONE launch does both (epg_pair_count_null_parts: a wave counts a tile of both groups, then draws its null groups -- the
        memory pipe and the VALU of a CU are busy at the same time without a second kernel).  Otherwise one launch for the
        count pass (epg_bin_hist_parts), then one for the null groups on the second stream (_start_null)."""
        eng, S = self.eng, self.S
        parts = [self.parts[pid] for pid, _na, _nb in batch]
        counts = self._acc() if self.sal == 1 else None  # counts over [A|B] = counts of A + counts of B (helpers.py:173)
        fused = None
        if self.groupSize == -1 and all(na == self.NA and nb == self.NB for _pid, na, nb in batch):
            fused = _unless_unsupported(eng.pair_count_null_parts, [p.XA for p in parts], [p.XB for p in parts], self.NA, self.NB, S,
                                        self.seed, [p.row0 for p in parts], counts=counts)
        if fused is not None:
            for p, HA, HB, HnA, HnB in zip(parts, *fused):
                p.HA, p.HB, p.HnA, p.HnB = HA, HB, HnA, HnB
        else:
            Hs, _ = eng.bin_hist_parts([p.XA for p in parts] + [p.XB for p in parts],
                                       [na for _pid, na, _nb in batch] + [nb for _pid, _na, nb in batch], S, counts=counts)
            for p, HA, HB in zip(parts, Hs, Hs[len(parts):]):
                p.HA, p.HB = HA, HB
        if self.sal == 2:
            for p in parts:
                eng.hist_s2_from_binhist_pair(p.HA, p.HB, S, counts=self._acc())
        if fused is None:
            self._start_null(parts)

    def _start_null(self, parts):
        """The null groups' histograms of `parts` (multivariate hypergeometric, from the real groups' histograms; they do not
        depend on exp_freq): one launch on the session's second stream, behind the launch that produced HA / HB.  Its outputs
        come from the main stream's pool (a second stream has a pool of its own in torch's allocator: every new session would
        start with device mallocs); the launch sits between two events, no stream switch on the host."""
        t = self.torch
        ga, gb = _null_widths(self.NA, self.NB, self.groupSize)
        ready = t.cuda.Event()
        ready.record(t.cuda.current_stream())
        self.null_stream.wait_event(ready)
        HnAs, HnBs = self.eng.null_hist_from_binhist_parts([p.HA for p in parts], [p.HB for p in parts], self.NA + self.NB, self.S,
                                                           ga, gb, self.seed, [p.row0 for p in parts], stream=self.null_stream)
        done = t.cuda.Event()
        done.record(self.null_stream)
        for x in (parts[0].HA, parts[0].HB, HnAs[0], HnBs[0]):
            x.record_stream(self.null_stream)            # used there: their memory must not be reused before it is through
        for p, HnA, HnB in zip(parts, HnAs, HnBs):
            p.HnA, p.HnB, p.null_done = HnA, HnB, done

    def _null_of(self, pid):
        """(HnA, HnB) of part `pid`, ready for the current stream."""
        self._flush()
        p = self.parts[pid]
        if p.null_done is not None:
            self.torch.cuda.current_stream().wait_event(p.null_done)
        return p.HnA, p.HnB

    # ---- multi-rank hand-over: the score pass of paired mode reads the two groups' histograms only
    n_export = 2

    def slice_part(self, pid, lo, hi, row0):
        self._flush()
        src = self.parts[pid]
        new = _Pair(None, None, _aligned_rows(src.HA, lo, hi), _aligned_rows(src.HB, lo, hi), row0)
        if src.HnA is not None:
            # the shuffle is keyed by (file, row in file): the rows' null groups are the ones drawn for the whole file
            HnA, HnB = self._null_of(pid)
            new.HnA, new.HnB = _aligned_rows(HnA, lo, hi), _aligned_rows(HnB, lo, hi)
        self.parts.append(new)
        return len(self.parts) - 1

    def export_rows(self, pid, lo, hi):
        self._flush()
        p = self.parts[pid]
        return [p.HA[lo:hi], p.HB[lo:hi]]

    def import_rows(self, tensors, widths, row0):
        self.NA, self.NB = widths
        p = _Pair(None, None, tensors[0].to(self.device), tensors[1].to(self.device), row0)
        self.parts.append(p)
        if p.HA.shape[0]:
            self._start_null([p])
        return len(self.parts) - 1

    def _results(self, pids):
        """{pid: device results} of the held parts among `pids`.  Paired S1 (the tables fit a CU's LDS): ONE launch of the fused
        pass over all the parts' histograms, quiescence masks included (epg_pair_scores_s1_parts) -- a launch per chromosome file
        paid the copy of the tables into LDS, the ramp and the tail 24 times (1.5 against 1.0 ms per 15 M bins).  Otherwise the
        separate passes, part by part (_separate)."""
        self._flush()
        pids = [pid for pid in pids if self.parts[pid] is not None]
        live = [pid for pid in pids if self.parts[pid].HA.shape[0]]
        out = {}
        if self.sal == 1 and live:
            NA, NB = self.NA, self.NB
            ga, gb = _null_widths(NA, NB, self.groupSize)
            tabs = [self._s1_table(n) for n in (NA, NB, ga, gb)]
            quads = [(self.parts[pid].HA, self.parts[pid].HB) + self._null_of(pid) for pid in live]
            out = dict(zip(live, _unless_unsupported(self.eng.pair_scores_s1_parts, quads, self.S, NA, NB, ga, gb, *tabs,
                                                     qstate=self.qstate) or []))
        res = {pid: out[pid] if pid in out else self._separate(pid) for pid in pids}
        if self.draws > 1:
            self._exceed(pids, res)
        return res

    @property
    def null_pool(self):
        """M, the size of the pooled null of the last exceedance pass: draws x the non-quiescent bins (synchronises)."""
        return 0 if self._null_kept is None else self.draws * int(self._null_kept.item())

    def _group_scores(self, H, n, N):
        """Scores of one group's histograms: its width n; S2 keeps the permutation count of the ORIGINAL group of width N (quirk
        Q9: the null halves, scores.py:397-398,418-421)."""
        if self.sal == 1:
            return self._score_s1(H, n)
        return self.eng.score_s2_from_binhist(H, max(n, N), self.S, self.q, perms=N * (N - 1))[0]

    def _null_dist(self, HnA, HnB):
        """The null distances of a part from its null groups' histograms, by the separate passes."""
        ga, gb = _null_widths(self.NA, self.NB, self.groupSize)
        return self.eng.pair_finish(self._group_scores(HnA, ga, self.NA), self._group_scores(HnB, gb, self.NB))[1]

    def _exceed(self, pids, res):
        """K = self.draws null draws per bin: res[pid]["exceed"][b] = #{x in pool : x >= |rdist[b]|}, int64, where the pool holds
        |null_k[b']| of every draw k (seed helpers.null_draw_seeds(seed, K)[k]: draw 0 is the run's own null) and every
        non-quiescent bin b' of the parts `pids` -- all the parts the session holds.  Runs once their real results exist.
        The draws go in chunks of whole draws whose buffers stay under null_chunk_bytes; every chunk is drawn (paired S1 of a
        state model: ONE launch of epg_null_dist_draws_parts, no null histogram in HBM; otherwise seed by seed with the calls of
        the K = 1 run), sorted once and counted into `exceed` (epg_null_exceed).  Quiescent bins are left out as NaN."""
        from .helpers import null_draw_seeds
        t, eng, S = self.torch, self.eng, self.S
        for pid in pids:
            res[pid]["exceed"] = t.zeros(res[pid]["rdist"].shape[0], dtype=t.int64, device=self.device)
        live = [pid for pid in pids if self.parts[pid].HA.shape[0]]
        self.null_chunks, self.null_fused = 0, None
        self._null_kept = t.zeros((), dtype=t.int64, device=self.device)
        if not live:
            return
        parts = [self.parts[pid] for pid in live]
        rows = [p.HA.shape[0] for p in parts]
        offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        Rtot = int(offs[-1])
        masks = [res[pid]["quies"] for pid in live]
        self._null_kept = Rtot - sum(m.sum(dtype=t.int64) for m in masks)
        d = t.cat([res[pid]["rdist"] for pid in live])
        exceed = t.zeros(Rtot, dtype=t.int64, device=self.device)
        seeds = null_draw_seeds(self.seed, self.draws)
        per = self.draws                                 # draws per chunk
        while per > 1 and 4 * per * Rtot + eng.null_exceed_ws_bytes(per * Rtot) > self.null_chunk_bytes:
            per -= 1
        flat = t.empty(per * Rtot, dtype=t.float32, device=self.device)
        ws = t.empty(eng.null_exceed_ws_bytes(per * Rtot), dtype=t.uint8, device=self.device)
        NA, NB = self.NA, self.NB
        ga, gb = _null_widths(NA, NB, self.groupSize)
        nan = float("nan")
        for k0 in range(0, self.draws, per):
            ks = seeds[k0:k0 + per]
            n = len(ks)
            outs = [flat[n * int(a):n * int(a + r)].view(n, r) for a, r in zip(offs, rows)]
            if self.null_fused is not False and self.sal == 1:
                got = _unless_unsupported(eng.null_dist_draws_parts, [p.HA for p in parts], [p.HB for p in parts], [p.row0 for p in parts],
                                          S, NA, NB, ga, gb, self._s1_table(ga), self._s1_table(gb), ks, masks=masks, outs=outs)
                self.null_fused = got is not None
            else:
                self.null_fused = False
            if not self.null_fused:
                for j, seed in enumerate(ks):
                    if k0 + j == 0:                      # the run's own null
                        nulls = [res[pid]["null"] for pid in live]
                    else:
                        HnAs, HnBs = eng.null_hist_from_binhist_parts([p.HA for p in parts], [p.HB for p in parts], NA + NB, S, ga, gb,
                                                                      int(seed), [p.row0 for p in parts])
                        nulls = [self._null_dist(HnA, HnB) for HnA, HnB in zip(HnAs, HnBs)]
                    for o, x, m in zip(outs, nulls, masks):
                        o[j].copy_(x)
                        o[j].masked_fill_(m.bool(), nan)
            eng.null_exceed(flat[:n * Rtot], d, exceed, ws=ws)
            self.null_chunks += 1
        for pid, a, r in zip(live, offs, rows):
            res[pid]["exceed"] = exceed[int(a):int(a) + r]

    def _separate(self, pid):
        """Scores of A, B and the two null groups, deltas, null distances, STEP 4's per-bin reduction and the quiescence mask
        of part `pid` from its resident histograms, one launch after another."""
        eng, S, NA, NB = self.eng, self.S, self.NA, self.NB
        HA, HB = self.parts[pid].HA, self.parts[pid].HB
        if HA.shape[0] == 0:
            t, dv = self.torch, self.device
            return {"delta": t.empty((0, S), dtype=t.float32, device=dv), "null": t.empty(0, dtype=t.float32, device=dv),
                    "quies": t.empty(0, dtype=t.uint8, device=dv), "rdist": t.empty(0, dtype=t.float32, device=dv),
                    "mdiff": t.empty(0, dtype=t.int32, device=dv)}
        HnA, HnB = self._null_of(pid)                    # (drawn straight from the real groups' when the part was counted)
        sA, sB = self._group_scores(HA, NA, NA), self._group_scores(HB, NB, NB)
        delta, _ = eng.pair_finish(sA, sB, want_dist=False)
        null = self._null_dist(HnA, HnB)
        rdist, mdiff = eng.pair_metrics(delta, roundtrip=True)     # what STEP 4 would recompute from the text
        quies = eng.quiescent_from_binhist(HA, NA, HB, NB, S, self.qstate)
        return {"delta": delta, "null": null, "quies": quies, "rdist": rdist, "mdiff": mdiff}

    def _begin(self, pids):
        self._early = self._results(pids)

    def _s1_widths(self):
        return [self.NA, self.NB] + ([self.groupSize] if self.groupSize != -1 else [])

    def results(self, pid, text=None):
        """Host arrays of part `pid`.  A part launch() did not score is scored with EVERY part still held (see _results); the
        parts are then downloaded one by one as the driver asks for them."""
        self.check()
        if pid not in self._early:
            self._early.update(self._results([p for p, part in enumerate(self.parts) if part is not None]))
            self._settle()
        r = self._early.pop(pid)
        out = {"null": r["null"].cpu().numpy(), "quies": r["quies"].cpu().numpy().astype(bool),
               "rdist": r["rdist"].cpu().numpy(), "mdiff": r["mdiff"].cpu().numpy()}
        # --writer gpu (text = the part's _io.Locations): the deltas become their file's BGZF bytes where they sit and are not
        # downloaded -- STEP 4 works from rdist and mdiff -- unless the device refused a value: then they come down for the host writer
        out["delta_text"] = None if text is None else self.device_text(text, r["delta"])
        if out["delta_text"] is None:
            self.downloaded["delta"] += 1
            out["delta"] = r["delta"].cpu().numpy()
        else:
            out["delta"] = None
        if text is None:
            del out["delta_text"]
        if "exceed" in r:                                # (--null-draws K > 1 only)
            out["exceed"] = r["exceed"].cpu().numpy()
        return out


def get():
    if _override is not None:
        return _override
    return HipBackend()


def set_for_testing(obj):
    """tests/ only."""
    global _override
    _override = obj
