"""Device plumbing: torch tensors (HBM buffers, streams) in, C-ABI calls out.  PyTorch is used only for
memory, streams and torch.distributed; every arithmetic step is a kernel of libepilogos_hip.so.

State matrices are int8 [R, ldx] with ldx = N rounded up to 16 bytes (pad bytes are never read as states), which
is the layout the streaming kernel's 16-byte loads want.  All functions enqueue on torch's current stream and
return device tensors without synchronising.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._abi import EpilogosHipError

ROW_ALIGN = 16


def require_gpu():
    if not torch.cuda.is_available():
        raise EpilogosHipError(-3, "no HIP device visible to torch: the epilogos_amd engine has no CPU fallback")
    _abi.load()


def ptr(t):
    """The unchecked address of a tensor (None: NULL) -- for the batch readers' launch-bound loops ("One binding per
    entry point") and for tests; every wrapper below hands its arguments to _arg / _mat instead."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(s=None):
    """The hipStream_t of the torch stream s (None: the current one)."""
    return C.c_void_p((torch.cuda.current_stream() if s is None else s).cuda_stream)


_ptr, _stream = ptr, stream


def aligned16(t):
    return t.data_ptr() % 16 == 0


# ---- the binding helpers: every wrapper's tensors go through _arg / _mat, its scratch through _scratch, its part tables through
# _parts / _ints.  They read tensor metadata only: no synchronisation, no device read, no launch (a captured graph never sees them).
def _on_device(where, t, dtype, dev):
    """What _arg and _mat ask of every tensor: on a CUDA device, the one of the call's other tensors, of the dtype the header names."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("engine.%s must be a tensor on a CUDA device" % where)
    if dev is not None and t.device != dev:
        raise ValueError("engine.%s is on %s, the call's other tensors on %s" % (where, t.device, dev))
    if t.dtype != dtype:
        raise ValueError("engine.%s must be %s, not %s" % (where, dtype, t.dtype))


def _arg(where, t, dtype, need, dev=None, null=False):
    """THE argument check, for a vector or flat buffer the kernel reads or writes `need` elements of: -> its address (NULL for None
    where `null` says the header documents one, and for a tensor without elements -- `need` is then 0).  where: "wrapper: argument";
    dev: the device of the call's other tensors.  A row slice H[a:b] is contiguous."""
    if t is None:
        if null:
            return None
        raise ValueError("engine.%s is required (the kernel takes no NULL pointer there)" % where)
    _on_device(where, t, dtype, dev)
    if not t.is_contiguous():
        raise ValueError("engine.%s must be contiguous (shape %s has strides %s)" % (where, tuple(t.shape), t.stride()))
    if t.numel() < need:                                         # (numel() again below: a tensor without elements has no address)
        raise ValueError("engine.%s holds %d elements, the kernel touches %d" % (where, t.numel(), need))
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _mat(where, t, dtype, width, dev=None):
    """_arg for a matrix the kernel takes with a row pitch (state matrices, format_scores' scores), of which it touches `width`
    columns: 2-D, unit column stride, a row stride of at least its width -> (address, rows, row pitch)."""
    _on_device(where, t, dtype, dev)
    if t.dim() != 2:
        raise ValueError("engine.%s must be 2-D" % where)
    R, W = t.shape
    if width > W:
        raise ValueError("engine.%s has rows of %d elements, the kernel touches %d" % (where, W, width))
    ld = t.stride(0)
    if R and ((W > 1 and t.stride(1) != 1) or (R > 1 and ld < W)):       # (a matrix without rows may have any strides)
        raise ValueError("engine.%s must have unit column stride and a row stride of at least its width (shape %s has strides %s)"
                         % (where, tuple(t.shape), t.stride()))
    return C.c_void_p(t.data_ptr()), R, max(ld, W)


def _scratch_bytes(entry, *dims, floor=256):
    """What the size query `entry` (a *_ws_bytes / *_bytes_max entry point; None: nothing to ask) answers for dims, at least `floor`."""
    return max(int(_abi.call(entry, *dims)) if entry else 0, floor)


def _scratch(where, ws, dev, entry, *dims):
    """THE scratch of a call: the caller's `ws` when given (a uint8 CUDA buffer; whether it is large enough is the library's
    EPG_ERR_WORKSPACE to say), else a fresh one of _scratch_bytes(entry, *dims) -> (buffer, address, bytes)."""
    if ws is None:
        ws = torch.empty(_scratch_bytes(entry, *dims), dtype=torch.uint8, device=dev)
    return ws, _arg(where, ws, torch.uint8, 0, dev), ws.numel()


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])


def _parts(where, ts, dtype, needs, dev):
    """_ptr_array of a multi-part call's tensors, each through _arg (entries may be None, and empty where their part has no rows)."""
    if len(ts) != len(needs):
        raise ValueError("engine.%s lists %d tensors for %d parts" % (where, len(ts), len(needs)))
    for t, need in zip(ts, needs):
        _arg(where, t, dtype, need, dev, null=True)
    return _ptr_array(ts)


def _ints(ctype, values):
    """The host array of a multi-part call's row counts, widths, pitches or keys."""
    return (ctype * len(values))(*[int(v) for v in values])


def padded_width(N):
    return (N + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def alloc_states(R, N, device="cuda"):
    """Uninitialised int8 [R, ldx] state matrix; use [:, :N]."""
    return torch.empty((R, padded_width(N)), dtype=torch.int8, device=device)


# ---- where the histogram cache of a RESIDENT matrix goes
PLACE_MIN_BYTES = 1 << 30           # a matrix under 1 GiB is counted in < 0.2 ms: not worth a probe
PLACE_BLOCK = 4 << 30               # candidates are the heads of blocks of this size (see alloc_hist)
PLACE_SEARCH_AT = 2                 # the n-th job on the same resident matrix runs the QUICK search ...
PLACE_TRIES = 8                     # ... at most 8 blocks (32 GiB: about what a process gets from the driver's pool of cleared memory at
PLACE_BUDGET_MS = 50.0              #     0.3 ms per block) and 50 ms of probe time
PLACE_DEEP_AT = 4                   # the n-th job, if the quick search kept the plain allocation, runs the DEEP search, once ...
PLACE_DEEP_TRIES = 24               # ... 24 blocks = 96 GiB, past what one memory class can span; memory beyond the cleared pool costs the
PLACE_DEEP_WALL_MS = 5000.0         #     driver ~30 ms per GiB to hand out (tools/alloc_probe.py): seconds, which only a process that keeps
                                    #     running jobs on the matrix gets back (0.3 ms per 15 M-bin job) -- hence the job count in front of it
PLACE_GAP = 0.03                    # two levels of the probe's ratio are "two memory classes" when they lie >= 3 % apart
PLACE_SURE = 1.10                   # K1 with the H store / K1 counts only at or under this: the store lands in another class, no
                                    # contrast needed (every block ever measured in the matrix's own class: >= 1.136; in another: 1.05-1.105)
PLACE_WIN = 0.01                    # the pick must beat the plain allocation by this much over the WHOLE matrix to replace it
_placement = {}                     # device index -> {"key", "home", "report", "stream", "seen", "tier"}


def _storage_users(t):
    """Tensors (views included) alive on t's storage, or None when this torch cannot tell (placement is then off)."""
    f = getattr(torch._C, "_storage_Use_Count", None)
    if f is None:
        return None
    return int(f(t.untyped_storage()._cdata)) - 1            # (the wrapper made by untyped_storage() counts as one)


def _probe_slices(R, rows=1 << 20):
    """Three row ranges of a matrix (head, middle, tail; a fifth of a genome in all) the class probe runs on: a matrix may
    straddle two memory classes, a histogram cache is good only if it is in neither.  Starts are multiples of 32 bins (whole
    super-tiles, 16-byte aligned histogram rows)."""
    m = min(rows, R // 3) // 32 * 32
    if m <= 0:
        return [(0, R)]
    return [(0, m), ((R - m) // 2 // 32 * 32, (R - m) // 2 // 32 * 32 + m), ((R - m) // 32 * 32, (R - m) // 32 * 32 + m)]


def _probe_ms(X, N, S, Hflat, counts, slices, reps=2):
    """Device time of k_bin_hist over `slices` of X, histogram rows into the same rows of the candidate `Hflat` (None = counts
    only); one untimed pass first."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    H = None if Hflat is None else Hflat[:X.shape[0] * S * 2].view(torch.int16).view(X.shape[0], S)
    for k in range(reps + 1):
        if k == 1:
            ev[0].record()
        for lo, hi in slices:
            bin_hist(X[lo:hi], N, S, counts=counts, H=None if H is None else H[lo:hi], want_hist=H is not None)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def place_decide(ratios, excluded=(), gap=PLACE_GAP, sure=PLACE_SURE):
    """The placement decision from the candidates' slice ratios alone (host logic; tests/test_host_logic.py plays sequences
    through it).  -> (index of the pick or None, verdict):
      "sure"         the lowest ratio is <= `sure`: its store lands in another class than the matrix whatever the others say;
      "two-levels"   the sorted ratios split into two groups at a RELATIVE step >= `gap` (the largest step counts): the groups are
                     two memory classes as this process sees them now -- no absolute level involved -- and the pick is the lowest
                     of the lower group;
      "one-level"    no such step: every candidate lies in one class (the matrix's or another: the probe cannot say) -- the pick
                     is the lowest, and the caller may walk on.
    `excluded`: candidates already found to straddle (confirmation failed) -- never picked, still part of the picture."""
    live = [i for i in range(len(ratios)) if i not in set(excluded)]
    if not live:
        return None, "none"
    order = sorted(live, key=lambda i: ratios[i])
    best = order[0]
    if ratios[best] <= sure:
        return best, "sure"
    allo = sorted(range(len(ratios)), key=lambda i: ratios[i])
    steps = [(ratios[allo[k + 1]] / ratios[allo[k]] - 1.0, k) for k in range(len(allo) - 1)]
    if steps:
        step, k = max(steps)
        if step >= gap:
            lower = [i for i in allo[:k + 1] if i not in set(excluded)]
            if lower:
                return lower[0], "two-levels"
    return best, "one-level"


def placement_enabled():
    """Off with EPILOGOS_PLACEMENT=0, when this torch cannot count a storage's users, and when the launcher put more ranks on the
    node than it has devices (ranks sharing a GPU -- run.py's gloo mode, tests -- must not each hold a home block and a cache of
    probe blocks)."""
    import os
    if os.environ.get("EPILOGOS_PLACEMENT", "1") == "0" or getattr(torch._C, "_storage_Use_Count", None) is None:
        return False
    try:
        lws = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    except ValueError:
        lws = 1
    return lws <= max(torch.cuda.device_count(), 1)


def _order_after_last_user(st):
    """The home is handed out again: whatever the previous holder enqueued on ITS stream must be over before this one's kernels
    write the block.  The views bypass torch's caching allocator, which would do this for an ordinary tensor: an event on the
    previous holder's stream, awaited by the current one (nothing when they are the same stream)."""
    prev, cur = st.get("stream"), torch.cuda.current_stream()
    if prev is not None and prev != cur:
        ev = torch.cuda.Event()
        ev.record(prev)
        cur.wait_event(ev)
    st["stream"] = cur


def alloc_hist(X, N, S):
    """The [R, S] uint16 histogram cache (int16 storage) for a RESIDENT state matrix X -- in another memory CLASS than X once
    the process has shown that it keeps running jobs on that matrix.

    The 288 GB of an MI355X fall into three classes of a third each (96 GB, contiguous in the driver's allocation order -- the
    three ranks of its 12-high HBM stacks would look exactly like this; profiles/r02ae_k1_memory_class_map.txt).  k_bin_hist
    reads X and writes H: with both in one class the launch is 13-17 % slower (2.6 against 2.3 ms for 15 M x 833) whatever the
    offsets, the data or the other buffers are.  HIP does not tell the class of an allocation, so the classifier is the kernel
    itself, on three 1 M-bin slices of X (head, middle, tail): ratio = launches with the H store into the candidate /
    counts-only launches.  Candidate 0 is the PLAIN allocation this function replaces (next to the matrix, as a rule in its
    class); the others are the heads of 4 GiB blocks allocated one after the other and held during the search, which makes the
    driver walk through its memory.  place_decide reads the ratios (a candidate at or under PLACE_SURE ends the walk at once;
    otherwise it goes on until two levels >= 3 % apart show, pick = the lowest of the lower one, or a bound is reached, pick =
    the lowest), and then ONE comparison decides, over the WHOLE matrix (the slices cover a fifth of it and miss a class
    boundary inside it): the pick against the plain allocation -- a pick that does not win by 1 % is set aside and the walk
    goes on; three losses end it.  The cache is therefore never slower than the plain allocation it replaces.

    What the search may cost is tied to what it can earn (0.3 ms per 15 M-bin job):
      * job 1 on a matrix: no search, a plain allocation -- a command-line run (one job per matrix) never pays anything;
      * job PLACE_SEARCH_AT: the QUICK search -- <= 8 blocks, <= 50 ms of probes, ended by the first block the driver is slow to
        hand out: 20-40 ms in all, 160 ms at worst.  About 32 GiB past the matrix come from the driver's pool of cleared memory
        at 0.3 ms per block; the class boundary lies inside that stretch for roughly a third of the fresh processes (it is
        96 GB away at most, anywhere with equal odds), and for another share the plain allocation is in another class already;
      * job PLACE_DEEP_AT, if the plain allocation was kept: the DEEP search, once -- <= 24 blocks (96 GiB, past any class),
        <= 5 s: beyond the cleared pool the driver takes ~30 ms per GiB to hand memory out, i.e. 1-3 s for the walk
        (tools/alloc_probe.py; profiles/r06d_alloc_probe.txt), which a process that keeps running jobs gets back and a single job does not.
    A block that wins is the device's HOME for the life of the process (H is a view of its head): later jobs on the same
    matrix get it without a probe, a job on another matrix after one probe.  The other blocks go back to torch's caching
    allocator (not to the driver: freed device memory is scrubbed in the background at every HBM-bound kernel's expense; torch
    reuses cached blocks and returns them by itself when an allocation would otherwise fail); the report says how much.
    While a view of the home is alive the next request gets a plain allocation; a hand-out on another stream than the previous
    one waits for that stream (_order_after_last_user).  release_placement() gives the home up.
    placement_enabled() says when all of this is off (plain allocations): EPILOGOS_PLACEMENT=0, ranks sharing a GPU.
    EPILOGOS_PLACEMENT_EAGER=1: both searches at the first job (tools, tests)."""
    import os
    R = X.shape[0]
    dev = X.device
    hbytes = R * S * 2
    plain = lambda: torch.empty((R, S), dtype=torch.int16, device=dev)
    if X.numel() < PLACE_MIN_BYTES or not placement_enabled():
        return plain()
    st = _placement.get(dev.index)
    stor = X.untyped_storage()
    key = (stor.data_ptr(), stor.nbytes())
    view = lambda home: home[:hbytes].view(torch.int16).view(R, S)
    eager = os.environ.get("EPILOGOS_PLACEMENT_EAGER") == "1"
    if st is not None and st["home"] is not None and st["home"].numel() >= hbytes:
        users = _storage_users(st["home"])
        if users is None or users > 1:
            st["report"]["plain_while_home_in_use"] = st["report"].get("plain_while_home_in_use", 0) + 1
            return plain()
        if st["key"] == key:
            st["report"]["reuses"] = st["report"].get("reuses", 0) + 1
            _order_after_last_user(st)
            return view(st["home"])
        counts = zeros_counts(S, device=dev)                 # another matrix: is the home good for it too?
        slices = _probe_slices(R)
        r = _probe_ms(X, N, S, st["home"], counts, slices) / _probe_ms(X, N, S, None, counts, slices)
        if r <= PLACE_SURE:
            st["key"] = key
            st["report"].update(revalidated=st["report"].get("revalidated", 0) + 1, ratio=round(r, 3))
            _order_after_last_user(st)
            return view(st["home"])
        st = None                                            # no: this matrix starts over (the old home goes to torch's cache)
        _placement.pop(dev.index, None)
    if st is None or st["key"] != key:
        st = _placement[dev.index] = {"key": key, "home": None, "report": {"jobs_seen": 0, "tier": "none yet"}, "stream": None, "seen": 0, "tier": 0}
    st["seen"] += 1
    st["report"]["jobs_seen"] = st["seen"]
    want = 0
    if st["tier"] < 1 and (eager or st["seen"] >= PLACE_SEARCH_AT):
        want = 1
    elif st["tier"] == 1 and (eager or st["seen"] >= PLACE_DEEP_AT):
        want = 2
    if not want:
        return plain()
    deep = want == 2
    home, h_plain, report = _place_search(X, N, S, int(os.environ.get("EPILOGOS_PLACEMENT_TRIES", PLACE_DEEP_TRIES if deep else PLACE_TRIES)),
                                          3 * PLACE_BUDGET_MS if deep else PLACE_BUDGET_MS, PLACE_DEEP_WALL_MS if deep else 10 * PLACE_BUDGET_MS,
                                          stop_at_slow_alloc=not deep)
    report.update(tier="deep" if deep else "quick", jobs_seen=st["seen"], reuses=0)
    if deep and "quick" not in report:
        report["quick"] = {k: st["report"].get(k) for k in ("decision", "ratios", "blocks_tried", "search_ms")}
    if home is None and report["picked"] == 0 and report["decision"].startswith("plain allocation kept (sure"):
        want = 2                                             # the plain allocation already lies in another class: nothing to look for
    st.update(home=home, report=report, stream=torch.cuda.current_stream(), tier=want)
    if home is None and eager and want == 1:
        return alloc_hist(X, N, S)                           # (eager: the deep search follows at once)
    return view(home) if home is not None else h_plain


PLACE_SLOW_ALLOC_MS = 20.0          # a 4 GiB block that takes longer to get comes from beyond the driver's pool of cleared memory


def _place_search(X, N, S, tries, budget_ms, wall_ms, stop_at_slow_alloc=False):
    """One search of alloc_hist: -> (home block or None = the plain allocation stays, the plain allocation, report).
    stop_at_slow_alloc (the quick search): the walk ends with the first block the driver takes more than PLACE_SLOW_ALLOC_MS to
    hand out -- every further one would cost the same ~120 ms."""
    import time
    R = X.shape[0]
    dev = X.device
    hbytes = R * S * 2
    t_start = time.perf_counter()
    counts = zeros_counts(S, device=dev)
    slices = _probe_slices(R)
    whole = [(0, R)]
    spent = [0.0]                                            # device time of the probes so far (ms)

    def probe(cand, where, reps=2):
        ms = _probe_ms(X, N, S, cand, counts, where, reps=reps)
        spent[0] += ms * (reps + 1)
        return ms

    base = probe(None, slices)
    block = max(PLACE_BLOCK, (hbytes + 4095) // 4096 * 4096)
    h_plain = torch.empty((R, S), dtype=torch.int16, device=dev)
    cands, ratios = [h_plain.view(torch.int8).view(-1)], []
    t0 = probe(cands[0], slices)
    base = min(base, probe(None, slices))                    # (the very first launches of a process run on a cold clock: the lower of two)
    ratios.append(t0 / base)
    whole_ms, excluded, alloc_ms = {}, [], []

    def walk_on():
        """One more block, probed on the slices; False when a bound is reached."""
        k = len(cands) - 1
        if k >= tries or spent[0] >= budget_ms or (time.perf_counter() - t_start) * 1e3 >= wall_ms:
            return False
        if stop_at_slow_alloc and alloc_ms and alloc_ms[-1] > PLACE_SLOW_ALLOC_MS:
            return False
        free, _total = torch.cuda.mem_get_info(dev)
        if free < block + 16 * hbytes + (8 << 30):           # the rest of the job must still fit
            return False
        t0 = time.perf_counter()
        try:
            cands.append(torch.empty(block, dtype=torch.int8, device=dev))
        except RuntimeError:
            return False
        torch.cuda.synchronize(dev)
        alloc_ms.append((time.perf_counter() - t0) * 1e3)
        ratios.append(probe(cands[-1], slices) / base)
        return True

    # walk until the slices decide (or a bound is reached), then the comparison that counts: the pick against the plain allocation
    # over the WHOLE matrix.  A pick that loses is set aside and the walk goes on from where it stopped (three such losses end it).
    pick, verdict = place_decide(ratios, excluded)
    while True:
        while verdict not in ("sure", "two-levels") and walk_on():
            pick, verdict = place_decide(ratios, excluded)
        if pick in (None, 0):
            break
        if slices == whole:
            whole_ms = {0: ratios[0] * base, pick: ratios[pick] * base}
        else:
            if 0 not in whole_ms:
                whole_ms[0] = probe(cands[0], whole, reps=1)
            whole_ms[pick] = probe(cands[pick], whole, reps=1)
        if whole_ms[pick] < whole_ms[0] * (1.0 - PLACE_WIN):
            break
        excluded.append(pick)
        if len(excluded) >= 3 or spent[0] >= 2 * budget_ms:
            pick = 0
            break
        pick, verdict = place_decide(ratios, excluded)
        verdict += " (after %d pick(s) that lost over the whole matrix)" % len(excluded)
    if pick is None or pick in excluded:
        pick = 0
    good = pick != 0
    report = {"probe": "k_bin_hist over 3 x %d bins of the matrix: with the H store into a candidate / counts only; candidate 0 is the plain "
                       "allocation, the others heads of %d GiB blocks allocated one after the other" % (slices[0][1] - slices[0][0], block >> 30),
              "decision": verdict if good else "plain allocation kept (%s)" % verdict, "good": good, "picked": pick, "ratio": round(ratios[pick], 3),
              "ratios": [round(r, 3) for r in ratios], "whole_matrix_ms": {str(i): round(v, 4) for i, v in whole_ms.items()},
              "lost_over_the_whole_matrix": excluded, "blocks_tried": len(cands) - 1,
              "walked_GiB": round(sum(c.numel() for c in cands[1:]) / 2**30, 1),
              "block_alloc_ms": [round(a, 1) for a in alloc_ms],
              "rules": {"sure_at_or_under": PLACE_SURE, "two_levels_apart_by": PLACE_GAP, "must_beat_plain_by": PLACE_WIN,
                        "max_blocks": tries, "max_probe_ms": budget_ms, "max_wall_ms": wall_ms},
              "ms_counts_only": round(base, 4), "probe_device_ms": round(spent[0], 2),
              "left_in_torch_cache_GiB": round(sum(c.numel() for i, c in enumerate(cands) if i and i != pick) / 2**30, 1)}
    home = cands[pick] if good else None
    del cands                                                # losing blocks -> torch's cache (not the driver)
    report["search_ms"] = round((time.perf_counter() - t_start) * 1e3, 2)
    return home, h_plain, report


def placement_report(device=None):
    """What alloc_hist did on this device (None: it never searched)."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    st = _placement.get(idx)
    return None if st is None else dict(st["report"])


def release_placement():
    """Forget the home (its memory goes to torch's cache; torch.cuda.empty_cache() then returns it and the probe blocks to the
    driver).  For a process that is done with resident-matrix jobs and wants the memory for something else."""
    _placement.clear()


def states_to_device(x, device="cuda"):
    """Host int array [R, N] of 0-based states -> padded int8 device matrix."""
    x = np.ascontiguousarray(x)
    R, N = x.shape
    ldx = padded_width(N)
    host = np.full((R, ldx), -1, dtype=np.int8)
    host[:, :N] = x.astype(np.int8)
    return torch.from_numpy(host).to(device)


def zeros_counts(n, dtype=torch.int64, device="cuda"):
    return torch.zeros(n, dtype=dtype, device=device)


def bin_hist(X, N, S, want_hist=True, counts=None, want_counts=True, H=None):
    """K1: per-bin histograms H uint16 [R, S] (as int16 storage) and/or counts[S] += column sums."""
    pX, R, ldx = _mat("bin_hist: X", X, torch.int8, N)
    dev = X.device
    if H is None and want_hist:
        H = torch.empty((R, S), dtype=torch.int16, device=dev)
    if want_counts and counts is None:
        counts = zeros_counts(S, device=dev)
    _abi.call("epg_bin_hist", pX, R, N, ldx, S, _arg("bin_hist: H", H, torch.int16, R * S, dev, null=True),
              _arg("bin_hist: counts", counts, torch.int64, S, dev, null=True) if want_counts else None, _stream())
    return H, counts


def bin_hist_s2(X, N, S, counts2=None, H=None, counts=None):
    """K1 with the S2 pair counts of the same bins folded into the launch (epg_bin_hist_s2): -> (H, counts2 int64 [S*S]);
    counts (int64 [S], optional) also gets the state counts."""
    pX, R, ldx = _mat("bin_hist_s2: X", X, torch.int8, N)
    dev = X.device
    if H is None:
        H = torch.empty((R, S), dtype=torch.int16, device=dev)
    if counts2 is None:
        counts2 = zeros_counts(S * S, device=dev)
    _abi.call("epg_bin_hist_s2", pX, R, N, ldx, S, _arg("bin_hist_s2: H", H, torch.int16, R * S, dev),
              _arg("bin_hist_s2: counts", counts, torch.int64, S, dev, null=True),
              _arg("bin_hist_s2: counts2", counts2, torch.int64, S * S, dev), _stream())
    return H, counts2


def hist_rows_flat(rows, S, device, dtype=torch.int16):
    """One allocation for the [R_p, S] rows of several parts: -> (flat [R_total_padded, S], starts).  Every part starts 16-byte
    aligned (its first row at a multiple of 8 rows: 8 rows of any S are a multiple of 16 bytes).  The <= 7 rows between two parts
    are never written by the count pass, and a score launch over the whole buffer scores them from whatever they hold: the lookup
    stays in bounds (k_score_s1_from_hist scores a count outside 1 .. N as 0) and their scores are never handed out."""
    starts, at = [], 0
    for r in rows:
        starts.append(at)
        at += (r + 7) // 8 * 8
    return torch.empty((max(at, 1), S), dtype=dtype, device=device), starts


def hist_rows_alloc(rows, S, device):
    """hist_rows_flat as a list of views, one per part."""
    flat, starts = hist_rows_flat(rows, S, device)
    return [flat[a:a + r] for a, r in zip(starts, rows)]


def bin_hist_parts(Xs, Ns, S, counts=None, want_hist=True, Hs=None):
    """K1 over several resident matrices in as few launches as their widths allow (epg_bin_hist_parts; one launch when all
    widths have the same number of 128-byte groups per row): -> (list of H [R_p, S] int16-stored uint16, counts), all parts'
    state counts added into the one `counts` (None: no counts)."""
    n = len(Xs)
    if n == 0:
        return [], counts
    dev = Xs[0].device
    shapes = [_mat("bin_hist_parts: Xs", X, torch.int8, N, dev)[1:] if X.shape[0] else (0, max(N, 1)) for X, N in zip(Xs, Ns)]
    rows = [r for r, _l in shapes]
    if Hs is None and want_hist:
        Hs = hist_rows_alloc(rows, S, dev)
    _abi.call("epg_bin_hist_parts", n, _ptr_array(Xs), _ints(C.c_int64, rows), _ints(C.c_int32, [N or 1 for N in Ns]),
              _ints(C.c_int64, [l for _r, l in shapes]),
              S, _parts("bin_hist_parts: Hs", Hs, torch.int16, [r * S for r in rows], dev) if Hs is not None else None,
              _arg("bin_hist_parts: counts", counts, torch.int64, S, dev, null=True), _stream())
    return Hs, counts


GROUPS_MAX = 4                      # EPG_GROUPS_MAX of include/epilogos_groups.h: column groups per launch
GROUPS_MAX_STATES = 31              # the grouped count pass serves the five-bit counting core; wider models gather (select_columns)
_members = {}                       # (device, N, groups as bytes) -> uint8 [N] membership tensor


def check_columns(cols, N):
    """A group's columns as a contiguous int64 array; 0-based, inside [0, N), no duplicates."""
    cols = np.ascontiguousarray(np.asarray(cols, dtype=np.int64).reshape(-1))
    if cols.size and (cols.min() < 0 or cols.max() >= N):
        raise ValueError("column index outside 0 .. %d" % (N - 1))
    if np.unique(cols).size != cols.size:
        raise ValueError("a column is listed twice in one group")
    return cols


def group_members(device, N, groups):
    """The membership tensor of epg_bin_hist_groups, uint8 [N]: bit g of byte c = column c belongs to groups[g].  Built once per
    (device, N, groups) and kept (a run passes the same groups for every part)."""
    groups = [check_columns(g, N) for g in groups]
    device = torch.device(device)
    key = (str(device), int(N), tuple(g.tobytes() for g in groups))
    m = _members.get(key)
    if m is None:
        host = np.zeros(N, dtype=np.uint8)
        for g, cols in enumerate(groups):
            host[cols] |= np.uint8(1 << g)
        if len(_members) >= 64:
            _members.clear()
        m = _members[key] = torch.from_numpy(host).to(device)
    return m


def forget_group_members():
    """Drop the kept membership tensors (a closed session's groups: a run of many groupings would otherwise leave one per
    grouping on the device until 64 have gathered)."""
    _members.clear()


def bin_hist_groups(X, N, S, groups, counts=None, want_hist=True):
    """The count pass for column groups of ONE matrix (epg_bin_hist_groups): X is read once, every group gets per-bin
    histograms of its own columns.  groups: 1 .. GROUPS_MAX int64 arrays of 0-based columns.  -> ([H_g uint16 [R, S] as int16
    storage] or None, counts int64 [G, S]; counts is added to when given)."""
    pX, R, ldx = _mat("bin_hist_groups: X", X, torch.int8, N)
    G, dev = len(groups), X.device
    member = group_members(dev, N, groups)
    Hs = hist_rows_alloc([R] * G, S, dev) if want_hist else None
    if counts is None:
        counts = zeros_counts(G * S, device=dev)
    _abi.call("epg_bin_hist_groups", pX, R, N, ldx, S, G, _arg("bin_hist_groups: member", member, torch.uint8, N, dev),
              _ptr_array(Hs) if Hs is not None else None, _arg("bin_hist_groups: counts", counts, torch.int64, G * S, dev), _stream())
    return Hs, counts.view(G, S)


FIRST_BAD_NONE = np.iinfo(np.int64).max     # what first_bad holds while no byte of the matrix is "not a state"


def state_census(X, N, S, census=None, other=None, first_bad=None, want_other=True, want_first_bad=True):
    """The per-biosample census of a state matrix (epg_state_census): -> (census int64 [N, S], other int64 [N], first_bad int64 [1]).
    census[n, s] = rows whose column n holds state s, other[n] = rows whose byte there is no state (the WHOLE byte is compared:
    0xFF, S .. 31 and the bytes 32 .. 254 that the count kernels would alias), first_bad = the smallest row * N + column of such a
    byte, FIRST_BAD_NONE when there is none.  Tensors given are added to (first_bad: minimised); want_other / want_first_bad
    False pass NULL and return None in their place."""
    pX, R, ldx = _mat("state_census: X", X, torch.int8, N)
    dev = X.device
    if census is None:
        census = torch.zeros((N, S), dtype=torch.int64, device=dev)
    if other is None and want_other:
        other = torch.zeros(N, dtype=torch.int64, device=dev)
    if first_bad is None and want_first_bad:
        first_bad = torch.full((1,), FIRST_BAD_NONE, dtype=torch.int64, device=dev)
    ptrs = [_arg("state_census: " + name, t, torch.int64, n, dev, null=null)
            for name, t, n, null in (("census", census, N * S, False), ("other", other, N, True), ("first_bad", first_bad, 1, True))]
    if census.numel() != N * S:                                  # (it is returned as [N, S])
        raise ValueError("engine.state_census: census must hold %d elements" % (N * S))
    if N > 0:                                                    # (an empty census tensor has no address to hand over)
        _abi.call("epg_state_census", pX, R, N, max(ldx, 1), S, *ptrs, _stream())
    return census.view(N, S), other, first_bad


def concordance_ws_bytes(R, N, S):
    return _scratch_bytes("epg_concordance_ws_bytes", R, N, S)


def concordance(X, N, S, agree=None, both=None, want_both=True, ws=None):
    """Pairwise state agreement of the biosample columns of a state matrix (epg_concordance): -> (agree, both), int64 [N, N].
    agree[i, j] = bins in which columns i and j hold the same state, both[i, j] = bins in which both hold a state (the WHOLE byte
    is compared, as in state_census); both triangles and the diagonal, agree[i, i] == both[i, i] == the valid bins of column i.
    Tensors given are added to; want_both False passes NULL and returns None in its place.  The workspace is sized and owned
    here unless `ws` (uint8, at least concordance_ws_bytes(R, N, S)) is handed in."""
    pX, R, ldx = _mat("concordance: X", X, torch.int8, N)
    dev = X.device
    if N < 1:
        raise ValueError("concordance needs at least one biosample column")
    if agree is None:
        agree = torch.zeros((N, N), dtype=torch.int64, device=dev)
    if both is None and want_both:
        both = torch.zeros((N, N), dtype=torch.int64, device=dev)
    ptrs = [_arg("concordance: " + name, t, torch.int64, N * N, dev, null=null) for name, t, null in (("agree", agree, False), ("both", both, True))]
    if agree.numel() != N * N or (both is not None and both.numel() != N * N):    # (they are returned as [N, N])
        raise ValueError("engine.concordance: agree and both must hold %d elements" % (N * N))
    if R > 0:
        _ws, pws, nws = _scratch("concordance: ws", ws, dev, "epg_concordance_ws_bytes", R, N, S)
        _abi.call("epg_concordance", pX, R, N, ldx, S, *ptrs, pws, nws, _stream())
    return agree.view(N, N), (both.view(N, N) if both is not None else None)


def gennorm_ws_bytes(M, T, n=0):
    return _scratch_bytes("epgf_gennorm_ws_bytes", M, T, n)


def _vector(where, x, dtype):
    """_arg for a non-empty 1-D input whose length is the call's size -> (address, length)."""
    p = _arg(where, x, dtype, 1)
    if x.dim() != 1:
        raise ValueError("engine.%s must be 1-D" % where)
    return p, x.numel()


def gennorm_fit(x, idx=None, n=None, ws=None):
    """T generalised-normal maximum-likelihood fits on the device (epgf_gennorm_fit, include/epilogos_gennorm.h): trial t fits
    x[idx[t]] (idx: int32 [T, n], every index in 0 .. M-1, checked here); idx None: one trial on all of x.
    -> (params float64 [T, 3] = (beta, loc, scale), fval float64 [T], info int32 [T, 2] = (evaluations, flag)); flag 0 converged,
    1 stopped at the cap, 2 degenerate sample (params NaN).  Current stream, no synchronisation beyond the index check's."""
    px, M = _vector("gennorm_fit: x", x, torch.float32)
    dev = x.device
    if idx is None:
        T, n, pidx = 1, M if n is None else int(n), None
    else:
        pidx = _arg("gennorm_fit: idx", idx, torch.int32, 1, dev)
        if idx.dim() != 2:
            raise ValueError("engine.gennorm_fit: idx must be 2-D [T, n]")
        T = idx.shape[0]
        if n is not None and int(n) != idx.shape[1]:
            raise ValueError("n=%d is not the row length %d of idx" % (n, idx.shape[1]))
        n = idx.shape[1]
        lo, hi = torch.aminmax(idx)
        if int(lo) < 0 or int(hi) >= M:
            raise ValueError("idx holds an index outside 0 .. %d" % (M - 1))
    params = torch.empty((T, 3), dtype=torch.float64, device=dev)
    fval = torch.empty(T, dtype=torch.float64, device=dev)
    info = torch.empty((T, 2), dtype=torch.int32, device=dev)
    _ws, pws, nws = _scratch("gennorm_fit: ws", ws, dev, "epgf_gennorm_ws_bytes", M, T, n)
    _abi.call("epgf_gennorm_fit", px, M, pidx, T, n, _ptr(params), _ptr(fval), _ptr(info), pws, nws, _stream())
    return params, fval, info


def gennorm_nnlf(x, params, ws=None):
    """Negative log-likelihood of ALL of x under each of the T parameter sets (epgf_gennorm_nnlf): params float64 [T, 3] ->
    float64 [T]; +inf for a set with beta <= 0, scale <= 0 or a NaN.  One pass over x."""
    px, M = _vector("gennorm_nnlf: x", x, torch.float32)
    dev = x.device
    pparams = _arg("gennorm_nnlf: params", params, torch.float64, 3, dev)
    if params.dim() != 2 or params.shape[1] != 3:
        raise ValueError("engine.gennorm_nnlf: params must be [T, 3]")
    T = params.shape[0]
    out = torch.empty(T, dtype=torch.float64, device=dev)
    _ws, pws, nws = _scratch("gennorm_nnlf: ws", ws, dev, "epgf_gennorm_ws_bytes", M, T, 0)
    _abi.call("epgf_gennorm_nnlf", px, M, pparams, T, _ptr(out), pws, nws, _stream())
    return out


def gennorm_pvals(x, params):
    """Two-sided p-value of every x under gennorm(beta, loc, scale) (epgf_gennorm_pvals, csrc/epg_pvals.h): params float64 [3] on
    the device, e.g. a row of gennorm_fit's.  -> (p float64 [M], flags int32 [2] = (NaN p-values, iterations stopped at the cap)).
    Current stream, no synchronisation."""
    px, M = _vector("gennorm_pvals: x", x, torch.float32)
    dev = x.device
    pparams = _arg("gennorm_pvals: params", params, torch.float64, 3, dev)
    if params.numel() != 3:
        raise ValueError("engine.gennorm_pvals: params must hold 3 elements (beta, loc, scale)")
    p = torch.empty(M, dtype=torch.float64, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    _abi.call("epgf_gennorm_pvals", px, M, pparams, _ptr(p), _ptr(flags), _stream())
    return p, flags


def bh_ws_bytes(M):
    return _scratch_bytes("epgf_bh_ws_bytes", M)


def bh_adjust(p, ws=None):
    """Benjamini-Hochberg adjusted p-values (epgf_bh_adjust), the bits of roiAndVisualPairwise.benjaminiHochberg: p float64 [M] ->
    (adj float64 [M], flags int32 [1] = the number of p that are NaN or negative; adj means nothing when it is not 0).  The
    workspace is sized and owned here unless `ws` (uint8, at least bh_ws_bytes(M)) is handed in.  Current stream, no synchronisation."""
    pp, M = _vector("bh_adjust: p", p, torch.float64)
    dev = p.device
    adj = torch.empty(M, dtype=torch.float64, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _ws, pws, nws = _scratch("bh_adjust: ws", ws, dev, "epgf_bh_ws_bytes", M)
    _abi.call("epgf_bh_adjust", pp, M, _ptr(adj), _ptr(flags), pws, nws, _stream())
    return adj, flags


# ---- the device text writer (csrc/epg_textout.h): epilogos --writer gpu
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
_text_bufs = {}                     # (device, name) -> uint8 tensor: ONE reusable set per device, grown when a part needs more


def _text_buf(device, name, nbytes):
    key = (str(device), name)
    t = _text_bufs.get(key)
    if t is None or t.numel() < nbytes:
        _text_bufs.pop(key, None)
        t = None                                             # (the smaller buffer goes before the larger one is asked for)
        t = _text_bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return t


def release_text_buffers():
    """Give the text writer's reusable buffers back (a session does when it closes)."""
    _text_bufs.clear()


def format_scores(scores, loc, loc_off, text=None, ws=None):
    """The text epgio_write_scores formats for float32 scores [R, S] (any row stride) and the rows' locations (loc uint8 blob, loc_off
    int64 [R + 1], both on the device), byte for byte (epgw_format_scores).  -> (text uint8, row_off int64 [R + 1], flags int32 [1]):
    the text is text[:row_off[R]]; nothing may be used when flags[0] != 0 (a value that is not finite or not below 2^31 in
    magnitude).  text / ws: buffers to use (None: allocated at their bounds).  Current stream, no synchronisation."""
    pscores, R, ld = _mat("format_scores: scores", scores, torch.float32, 1)
    S, dev = int(scores.shape[1]), scores.device
    ploc = _arg("format_scores: loc", loc, torch.uint8, 0, dev)
    ploc_off = _arg("format_scores: loc_off", loc_off, torch.int64, R + 1, dev)
    if loc_off.numel() != R + 1:
        raise ValueError("engine.format_scores: loc_off must hold R + 1 = %d elements" % (R + 1))
    text, ptext, ntext = _scratch("format_scores: text", text, dev, "epgw_text_bytes_max", R, S, loc.numel())
    _ws, pws, nws = _scratch("format_scores: ws", ws, dev, "epgw_format_ws_bytes", R)
    row_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call("epgw_format_scores", pscores if R else None, R, S, ld if R > 1 else S, ploc if R else None, ploc_off if R else None, ptext, ntext,
              _ptr(row_off), _ptr(flags), pws, nws, _stream())
    return text, row_off, flags


def bgzf_compress(text, n, row_off=None, eof=True, out=None, ws=None):
    """text[:n] (uint8, device) as BGZF (epgw_bgzf_compress): blocks of at most 65 280 text bytes, each its own gzip member, the
    28-byte end-of-file block behind them when `eof`.  row_off (int64 [R + 1], format_scores') lets the compressor match rows against
    the row above; without it only literals are coded.  -> (out uint8, n_out int64 [1], flags int32 [1]): the stream is
    out[:n_out].  Current stream, no synchronisation."""
    n = int(n)
    ptext = _arg("bgzf_compress: text", text, torch.uint8, n)
    dev = text.device
    R = 0 if row_off is None else row_off.numel() - 1
    prow_off = _arg("bgzf_compress: row_off", row_off, torch.int64, 0, dev, null=True)
    out, pout, nout = _scratch("bgzf_compress: out", out, dev, "epgw_bgzf_bytes_max", n, int(bool(eof)))
    _ws, pws, nws = _scratch("bgzf_compress: ws", ws, dev, "epgw_bgzf_ws_bytes", n)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call("epgw_bgzf_compress", ptext, n, prow_off if R else None, R, int(bool(eof)), pout, nout, _ptr(n_out), _ptr(flags), pws, nws, _stream())
    return out, n_out, flags


def _compress_formatted(text, row_off, flags, rows, ws, eof):
    """What format_scores / format_metrics just left in (text, row_off, flags) for `rows` rows, compressed by bgzf_compress into the
    device's "out" buffer -> (out, n_bytes); None when a format flag is set.  Synchronises twice: the text's size comes back between
    the two kernels' calls (the synchronisation csrc/epg_textout.h documents), the stream's size after them."""
    n, flag = (int(v) for v in torch.stack([row_off[rows], flags[0].to(torch.int64)]).cpu())
    if flag:
        return None
    out = _text_buf(text.device, "out", _scratch_bytes("epgw_bgzf_bytes_max", n, int(bool(eof))))
    out, n_out, flags = bgzf_compress(text, n, row_off, eof=eof, out=out, ws=ws)
    n_bytes, flag = (int(v) for v in torch.stack([n_out[0], flags[0].to(torch.int64)]).cpu())
    if flag:
        raise EpilogosHipError(-3, "the BGZF stream did not fit its own bound")
    return out, n_bytes


def scores_text_bgzf(locations, scores_device, eof=False):
    """A part's score file on the device: the text of format_scores for `locations` (a _io.Locations, uploaded here) and the float32
    [R, S] scores where they sit, compressed by bgzf_compress -> (uint8 device tensor, n_bytes): the file's bytes are the first
    n_bytes (without the end-of-file block unless `eof`: driver.finish_bgzf appends the one a finished file carries).  None when a
    flag is set -- a value the device does not format -- and nothing may be used: the caller writes that file on the host.
    Synchronises twice: the text's size comes back between the two kernels' calls (the synchronisation csrc/epg_textout.h
    documents), the stream's size after them.  The buffers are one reusable set per device (release_text_buffers)."""
    _p, R, _ld = _mat("scores_text_bgzf: scores_device", scores_device, torch.float32, 1)
    S = int(scores_device.shape[1])
    if len(locations) != R:
        raise ValueError("locations and scores disagree on the number of rows")
    dev = scores_device.device
    blob = np.ascontiguousarray(locations.blob, dtype=np.uint8)
    off = np.ascontiguousarray(locations.offsets, dtype=np.int64)
    loc = torch.from_numpy(blob).to(dev) if blob.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    loc_off = torch.from_numpy(off).to(dev)
    text = _text_buf(dev, "text", _scratch_bytes("epgw_text_bytes_max", R, S, int(off[-1] - off[0]) if R else 0))
    ws = _text_buf(dev, "ws", max(_scratch_bytes("epgw_format_ws_bytes", R), _scratch_bytes("epgw_bgzf_ws_bytes", text.numel())))
    text, row_off, flags = format_scores(scores_device, loc, loc_off, text=text, ws=ws)
    return _compress_formatted(text, row_off, flags, R, ws, eof)


# ---- the device metrics writer (csrc/epg_metrics_text.h): epilogos --metrics gpu
METRICS_CHUNK_TEXT_BYTES = 256 << 20    # a chunk of rows is formatted into at most this much text (its bound, not its size): with the
#                                         compressed stream's bound and the row arrays a chunk's buffers stay under 1 GiB


def _name_table(names, device):
    """A list of names as the blob and the int64 offsets the kernels read -> (blob uint8 device, off int64 device, bytes, longest)."""
    from . import _io
    blob, off = _io._string_table(names)                     # (the host writer's own tables; the blob ends in one spare byte)
    return torch.from_numpy(blob).to(device), torch.from_numpy(off).to(device), int(off[-1]), int(np.diff(off).max()) if len(off) > 1 else 0


def format_metrics(chrom, chrom_off, chrom_bytes, chrom_idx, start, end, names, names_off, names_bytes, maxdiff, dist, pvals=None, mh=None,
                   text=None, ws=None, chrom_max=None, name_max=None):
    """The rows epgio_write_metrics formats, byte for byte (epgm_format_metrics): chrom / names are the two name tables (uint8 blob of
    chrom_bytes / names_bytes bytes and int64 offsets, on the device), chrom_idx int32 [R], start / end int64 [R], maxdiff int32 [R]
    (1-based), dist float32 [R] and, both or neither, pvals / mh float64 [R] -- all contiguous, on one device.  -> (text uint8,
    row_off int64 [R + 1], flags int32 [1]): the text is text[:row_off[R]]; nothing may be used when flags[0] != 0 (the EPGM_FLAG_*
    bits of the header).  text / ws: buffers to use (None: allocated at their bounds, for names of at most chrom_max / name_max
    bytes, by default the header's EPGM_NAME_MAX).  Current stream, no synchronisation."""
    if (pvals is None) != (mh is None):
        raise ValueError("pvals and mh go together")
    pdist, R = _arg("format_metrics: dist", dist, torch.float32, 0), int(dist.numel())
    dev = dist.device
    def arg(name, t, dtype, need, null=False):                   # (checked whatever R is; the kernel gets NULL when there are no rows)
        p = _arg("format_metrics: " + name, t, dtype, need, dev, null)
        return p if R else None
    row = lambda name, t, dtype, null=False: arg(name, t, dtype, R, null)
    tab = lambda name, t, dtype: arg(name, t, dtype, int(dtype == torch.int64))
    if text is None:
        limit = _abi.header_constant_of(_abi.METRICS["metrics_text"], "EPGM_NAME_MAX")
        text = torch.empty(_scratch_bytes("epgm_text_bytes_max", R, limit if chrom_max is None else int(chrom_max),
                                          limit if name_max is None else int(name_max), int(pvals is not None)), dtype=torch.uint8, device=dev)
    text, ptext, ntext = _scratch("format_metrics: text", text, dev, None)
    _ws, pws, nws = _scratch("format_metrics: ws", ws, dev, "epgm_format_ws_bytes", R)
    row_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call("epgm_format_metrics", tab("chrom", chrom, torch.uint8), tab("chrom_off", chrom_off, torch.int64), chrom_off.numel() - 1,
              int(chrom_bytes), row("chrom_idx", chrom_idx, torch.int32), row("start", start, torch.int64), row("end", end, torch.int64),
              tab("names", names, torch.uint8), tab("names_off", names_off, torch.int64), names_off.numel() - 1, int(names_bytes),
              row("maxdiff", maxdiff, torch.int32), pdist if R else None, row("pvals", pvals, torch.float64, True), row("mh", mh, torch.float64, True),
              R, ptext, ntext, _ptr(row_off), _ptr(flags), pws, nws, _stream())
    return text, row_off, flags


def metrics_text_bgzf(chromNames, chrom_idx, start, end, stateNames, maxdiff, dist, pvals=None, mh=None, device=None):
    """pairwiseMetrics_*.txt.gz on the device: the rows of format_metrics, compressed by bgzf_compress, chunk of rows after chunk of rows
    -> a list of uint8 host arrays, the file's bytes without the end-of-file block (driver.write_bgzf appends the one a finished file
    carries); None when a flag is set -- a value or an index the device does not format -- and nothing may be used: the caller writes
    the file on the host.  The two name lists and the row arrays are host arrays (uploaded here, a chunk at a time); pvals and mh may be
    float64 device tensors instead (--pvals gpu leaves them there: no second upload).  Rows per chunk: as many as keep the bound of
    the chunk's text under METRICS_CHUNK_TEXT_BYTES.  Synchronises twice per chunk, as scores_text_bgzf does, and reuses its
    per-device buffers (release_text_buffers)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    R = len(dist)
    chrom, chrom_off, chrom_bytes, chrom_max = _name_table(chromNames, dev)
    names, names_off, names_bytes, name_max = _name_table(stateNames, dev)
    limit = _abi.header_constant_of(_abi.METRICS["metrics_text"], "EPGM_NAME_MAX")
    if chrom_max > limit or name_max > limit:
        return None
    with_p = pvals is not None
    per_row = _scratch_bytes("epgm_text_bytes_max", 1, chrom_max, name_max, int(with_p), floor=1)
    step = max(METRICS_CHUNK_TEXT_BYTES // per_row, 1)

    def up(a, lo, hi, dtype):
        if torch.is_tensor(a):
            return a[lo:hi].contiguous()
        return torch.from_numpy(np.ascontiguousarray(a[lo:hi], dtype=dtype)).to(dev)
    pieces = []
    for lo in range(0, R, step):
        hi = min(R, lo + step)
        n_rows = hi - lo
        text = _text_buf(dev, "text", per_row * n_rows)
        ws = _text_buf(dev, "ws", max(_scratch_bytes("epgm_format_ws_bytes", n_rows), _scratch_bytes("epgw_bgzf_ws_bytes", text.numel())))
        text, row_off, flags = format_metrics(chrom, chrom_off, chrom_bytes, up(chrom_idx, lo, hi, np.int32), up(start, lo, hi, np.int64),
                                              up(end, lo, hi, np.int64), names, names_off, names_bytes, up(maxdiff, lo, hi, np.int32),
                                              up(dist, lo, hi, np.float32), up(pvals, lo, hi, np.float64) if with_p else None,
                                              up(mh, lo, hi, np.float64) if with_p else None, text=text, ws=ws)
        done = _compress_formatted(text, row_off, flags, n_rows, ws, False)
        if done is None:
            return None
        pieces.append(done[0][:done[1]].cpu().numpy())
    return pieces


# ---- the device BGZF reader (csrc/epg_bgzf_inflate.h): simsearch --inflate gpu
def bgzf_inflate(comp, table, out=None, status=None, flags=None):
    """The members of a BGZF stream inflated on the device (epgz_bgzf_inflate): comp uint8 (device) holds the compressed bytes, table
    int64 [M, 5] (device; bgzfIndex.members' rows: payload offset in comp, payload bytes, text offset in out, ISIZE, CRC-32) says
    where every member lies and goes.  -> (out uint8, status int32 [M], flags int32 [1]): status[m] is 0 or the reason member m was
    given up (then its bytes of out are zeros), flags[0] the number of members with a reason.  out: the buffer to fill (None: one
    of max(text offset + ISIZE) bytes, which costs a synchronisation).  Current stream, no synchronisation otherwise."""
    pcomp, dev = _arg("bgzf_inflate: comp", comp, torch.uint8, 0), comp.device
    ptable = _arg("bgzf_inflate: table", table, torch.int64, 0, dev)
    if table.dim() != 2 or table.shape[1] != 5:
        raise ValueError("engine.bgzf_inflate: table must be [M, 5]")
    M = int(table.shape[0])
    if out is None:
        out = torch.empty(max(int((table[:, 2] + table[:, 3]).max()) if M else 0, 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(M, 1), dtype=torch.int32, device=dev)[:M]
    if flags is None:
        flags = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.call("epgz_bgzf_inflate", pcomp, comp.numel(), ptable, M, _arg("bgzf_inflate: out", out, torch.uint8, 0, dev), out.numel(),
              _arg("bgzf_inflate: status", status, torch.int32, M, dev), _arg("bgzf_inflate: flags", flags, torch.int32, 1, dev), _stream())
    return out, status, flags


def newline_index(text, seg_bytes, n=None):
    """Per segment of seg_bytes bytes (a multiple of 16) of text[:n] (uint8, device, 16-byte aligned): the number of newlines in it and
    the offset of the last one, -1 when there is none (epgz_newline_index) -> (count int64 [segments], last int64 [segments]).
    Current stream, no synchronisation."""
    ptext = _arg("newline_index: text", text, torch.uint8, 0 if n is None else int(n))
    n = text.numel() if n is None else int(n)
    both = torch.empty((2, _scratch_bytes("epgz_newline_segments", n, int(seg_bytes), floor=0)), dtype=torch.int64, device=text.device)
    _abi.call("epgz_newline_index", ptext if n else None, n, int(seg_bytes), _ptr(both[0]) if n else None, _ptr(both[1]) if n else None, _stream())
    return both[0], both[1]


def select_columns(X, cols):
    """The columns `cols` (0-based int64) of a state matrix as a matrix of its own: int8 [R, padded_width(len(cols))], padding
    bytes 0xFF.  What the grouped count pass does not serve (S3 needs the states themselves; models of 32 .. 127 states) runs
    the ordinary path on this.  A device gather, no host copy."""
    cols = check_columns(cols, X.shape[1])
    n = int(cols.size)
    out = torch.full((X.shape[0], padded_width(max(n, 1))), -1, dtype=torch.int8, device=X.device)
    if n:
        out[:, :n].copy_(torch.index_select(X, 1, torch.from_numpy(cols).to(X.device)))
    return out


def _rows(where, H, S, dev=None, dtype=torch.int16):
    """_arg for a [R, S] array whose row count is the call's R (a histogram, as a rule) -> (address, R)."""
    R = H.shape[0] if isinstance(H, torch.Tensor) and H.dim() else 0
    return _arg(where, H, dtype, R * S, dev), R


def null_hist_from_binhist_parts(HAs, HBs, n_cols, S, ga, gb, seed, row0s, stream=None):
    """epg_null_hist_from_binhist for several parts in one launch (bit-identical to a call per part); outputs from ONE allocation
    per group.  -> (list of OA, list of OB)."""
    n = len(HAs)
    if n == 0:
        return [], []
    rows = [h.shape[0] for h in HAs]
    dev = HAs[0].device
    need = [r * S for r in rows]
    pA, pB = _parts("null_hist_from_binhist_parts: HAs", HAs, torch.int16, need, dev), _parts("null_hist_from_binhist_parts: HBs", HBs, torch.int16, need, dev)
    OAs, OBs = hist_rows_alloc(rows, S, dev), hist_rows_alloc(rows, S, dev)
    _abi.call("epg_null_hist_from_binhist_parts", n, pA, pB, _ints(C.c_int64, rows), S, n_cols, ga, gb, seed, _ints(C.c_int64, row0s),
              _ptr_array(OAs), _ptr_array(OBs), _stream(stream))
    return OAs, OBs


def null_dist_draws_parts(HAs, HBs, row0s, S, NA, NB, ga, gb, TnA, TnB, seeds, masks=None, outs=None):
    """K null distances per bin of several parts in one launch (epg_null_dist_draws_parts, include/epilogos_nulldraws.h):
    -> list of float32 [K, R_p]; row k is the null distance that null_hist_from_binhist_parts with seeds[k] and
    pair_scores_s1_parts give.  masks: uint8 [R_p] per part (or None): masked rows are not drawn and hold NaN.  outs: the
    caller's [K, R_p] buffers.  Raises EpilogosHipError(-2) for shapes outside the kernel's: the two calls give the same."""
    n = len(HAs)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    K = int(seeds.size)
    rows = [h.shape[0] for h in HAs]
    dev = HAs[0].device if n else None
    if outs is None:
        outs = [torch.empty((K, r), dtype=torch.float32, device=dev or "cuda") for r in rows]
    w, need = "null_dist_draws_parts: ", [r * S for r in rows]
    _abi.call("epg_null_dist_draws_parts", n, _parts(w + "HAs", HAs, torch.int16, need, dev), _parts(w + "HBs", HBs, torch.int16, need, dev),
              _ints(C.c_int64, rows), _ints(C.c_int64, row0s), _parts(w + "masks", masks, torch.uint8, rows, dev) if masks is not None else None,
              S, NA, NB, ga, gb, _arg(w + "TnA", TnA, torch.float32, (ga + 1) * S, dev), _arg(w + "TnB", TnB, torch.float32, (gb + 1) * S, dev),
              seeds.ctypes.data_as(C.c_void_p), K, _parts(w + "outs", outs, torch.float32, [K * r for r in rows], dev), _stream())
    return outs


def null_exceed_ws_bytes(n):
    return _scratch_bytes("epg_null_exceed_ws_bytes", int(n))


def null_exceed(null, d, exceed, ws=None):
    """exceed[b] += #{x in null : x is not NaN and |x| >= |d[b]|} (epg_null_exceed): null float32 [n] (any shape, contiguous), d
    float32 [R], exceed int64 [R], accumulated into.  ws: uint8 workspace of null_exceed_ws_bytes(n) bytes (None: allocated)."""
    pnull, dev = _arg("null_exceed: null", null, torch.float32, 0), null.device
    pd = _arg("null_exceed: d", d, torch.float32, 0, dev)
    n, R = null.numel(), d.numel()
    pexceed = _arg("null_exceed: exceed", exceed, torch.int64, R, dev)
    if n == 0 or R == 0:
        return exceed
    _ws, pws, nws = _scratch("null_exceed: ws", ws, dev, "epg_null_exceed_ws_bytes", n)
    _abi.call("epg_null_exceed", pnull, n, pd, R, pexceed, pws, nws, _stream())
    return exceed


def pair_count_null_parts(XAs, XBs, NA, NB, S, seed, row0s, counts=None):
    """Paired mode, default group sizes: count pass of both groups and the null draw of several resident parts in ONE launch
    (epg_pair_count_null_parts).  -> (HAs, HBs, OAs, OBs) lists of [R_p, S] histograms (real groups, null groups).  Raises
    EpilogosHipError(-2) for shapes outside the fused kernel's: bin_hist_parts + null_hist_from_binhist_parts give the same."""
    n = len(XAs)
    dev = XAs[0].device
    sa = [_mat("pair_count_null_parts: XAs", X, torch.int8, NA, dev)[1:] if X.shape[0] else (0, padded_width(NA)) for X in XAs]
    sb = [_mat("pair_count_null_parts: XBs", X, torch.int8, NB, dev)[1:] if X.shape[0] else (0, padded_width(NB)) for X in XBs]
    rows = [r for r, _l in sa]
    if rows != [r for r, _l in sb]:
        raise ValueError("paired inputs must have the same number of bins")
    H = hist_rows_alloc(rows + rows, S, dev)
    O = hist_rows_alloc(rows + rows, S, dev)
    _abi.call("epg_pair_count_null_parts", n, _ptr_array(XAs), _ptr_array(XBs), _ints(C.c_int64, rows), NA, NB,
              _ints(C.c_int64, [l for _r, l in sa]), _ints(C.c_int64, [l for _r, l in sb]), S, _ptr_array(H[:n]), _ptr_array(H[n:]),
              _arg("pair_count_null_parts: counts", counts, torch.int64, S, dev, null=True), seed, _ints(C.c_int64, row0s), _ptr_array(O[:n]),
              _ptr_array(O[n:]), _stream())
    return H[:n], H[n:], O[:n], O[n:]


def hist_s2_from_binhist(H, S, counts=None):
    pH, R = _rows("hist_s2_from_binhist: H", H, S)
    if counts is None:
        counts = zeros_counts(S * S, device=H.device)
    _abi.call("epg_hist_s2_from_binhist", pH, R, S, _arg("hist_s2_from_binhist: counts", counts, torch.int64, S * S, H.device), _stream())
    return counts


def hist_s2_from_binhist_pair(HA, HB, S, counts=None):
    """S2 counts of the column concatenation [A|B] from the two groups' histograms (helpers.py:173)."""
    pHA, R = _rows("hist_s2_from_binhist_pair: HA", HA, S)
    pHB = _arg("hist_s2_from_binhist_pair: HB", HB, torch.int16, R * S, HA.device)
    if HA.shape != HB.shape:
        raise ValueError("paired histograms must have the same shape")
    if counts is None:
        counts = zeros_counts(S * S, device=HA.device)
    _abi.call("epg_hist_s2_from_binhist_pair", pHA, pHB, R, S, _arg("hist_s2_from_binhist_pair: counts", counts, torch.int64, S * S, HA.device),
              _stream())
    return counts


def hist_s3_ws_bytes(R, N, S):
    return _scratch_bytes("epg_ws_bytes", 3, R, N, S)


def hist_s3(X, N, S, counts=None, use_workspace=True, ws=None):
    """counts int32 [N*N*S*S] += biosample-pair state co-occurrences.  With a workspace (room for the transposed matrix)
    the matrix-core kernel runs; without one the ABI falls back to the LDS-counter kernel (same integers).  `ws`: a
    caller-owned workspace of at least hist_s3_ws_bytes(R, N, S) bytes (a session reuses one for all its parts)."""
    pX, R, ldx = _mat("hist_s3: X", X, torch.int8, N)
    dev = X.device
    if counts is None:
        counts = zeros_counts(N * N * S * S, dtype=torch.int32, device=dev)
    pws, nws = _scratch("hist_s3: ws", ws, dev, "epg_ws_bytes", 3, R, N, S)[1:] if use_workspace else (None, 0)
    _abi.call("epg_hist_s3", pX, R, N, ldx, S, _arg("hist_s3: counts", counts, torch.int32, N * N * S * S, dev), pws, nws, _stream())
    return counts


def normalise(counts, q=None, ws=None):
    """q = float32(counts / sum(counts)) on device (expectedCombination.py:42)."""
    name = {torch.int64: "epg_normalise_i64", torch.int32: "epg_normalise_i32"}.get(getattr(counts, "dtype", None))
    if name is None:
        raise ValueError("engine.normalise: counts must be an int64 or int32 tensor")
    pcounts, n, dev = _arg("normalise: counts", counts, counts.dtype, 0), counts.numel(), counts.device
    if q is None:
        q = torch.empty(n, dtype=torch.float32, device=dev)
    _ws, pws, nws = _scratch("normalise: ws", ws, dev, None)
    _abi.call(name, pcounts, n, _arg("normalise: q", q, torch.float32, n, dev), pws, nws, _stream())
    return q


def _outs(where, R, S, dev, want32, want64, out32=None, out64=None):
    """The two score outputs of a call, [R, S] each: given, allocated when wanted, or None -> (out32, out64, address of out64, of out32)."""
    o32 = out32 if out32 is not None else (torch.empty((R, S), dtype=torch.float32, device=dev) if want32 else None)
    o64 = out64 if out64 is not None else (torch.empty((R, S), dtype=torch.float64, device=dev) if want64 else None)
    return (o32, o64, _arg(where + ": out64", o64, torch.float64, R * S, dev, null=True),
            _arg(where + ": out32", o32, torch.float32, R * S, dev, null=True))


def workspace(saliency, R, N, S, device="cuda"):
    """Caller-owned scratch for the score calls of one saliency (tables; plus a histogram cache when R > 0)."""
    return torch.empty(_scratch_bytes("epg_ws_bytes", saliency, R, N, S), dtype=torch.uint8, device=device)


def score_s1(X, N, S, q, want32=True, want64=False, out32=None, out64=None, ws=None):
    pX, R, ldx = _mat("score_s1: X", X, torch.int8, N)
    dev = X.device
    o32, o64, p64, p32 = _outs("score_s1", R, S, dev, want32, want64, out32, out64)
    _ws, pws, nws = _scratch("score_s1: ws", ws, dev, "epg_ws_bytes", 1, R, N, S)
    _abi.call("epg_score_s1", pX, R, N, ldx, S, _arg("score_s1: q", q, torch.float32, S, dev), p64, p32, pws, nws, _stream())
    return o32, o64


def score_s1_from_binhist(H, N, S, q, want32=True, want64=False, out32=None, out64=None, ws=None):
    pH, R = _rows("score_s1_from_binhist: H", H, S)
    dev = H.device
    o32, o64, p64, p32 = _outs("score_s1_from_binhist", R, S, dev, want32, want64, out32, out64)
    _ws, pws, nws = _scratch("score_s1_from_binhist: ws", ws, dev, "epg_ws_bytes", 1, 0, N, S)
    _abi.call("epg_score_s1_from_binhist", pH, R, N, S, _arg("score_s1_from_binhist: q", q, torch.float32, S, dev), p64, p32, pws, nws, _stream())
    return o32, o64


def score_s1_from_binhist_table(H, N, S, T64=None, T32=None, out32=None, out64=None):
    """S1 scores of cached histograms from a caller-built table T[c, s], c = 0..N (device tensors [N + 1, S]; T32 -> float32
    scores, T64 -> float64 scores).  scores.s1ScoreTable builds the pair on the host with the reference's arithmetic."""
    w = "score_s1_from_binhist_table"
    pH, R = _rows(w + ": H", H, S)
    dev = H.device
    pT64 = _arg(w + ": T64", T64, torch.float64, (N + 1) * S, dev, null=True)
    pT32 = _arg(w + ": T32", T32, torch.float32, (N + 1) * S, dev, null=True)
    o32, o64, p64, p32 = _outs(w, R, S, dev, T32 is not None, T64 is not None, out32, out64)
    _abi.call("epg_score_s1_from_binhist_table", pH, R, N, S, pT64, pT32, p64, p32, _stream())
    return o32, o64


def combine_score_s1(counts, H, N, S, q=None, want32=True, want64=False, out32=None, out64=None, ws=None, rezero=False):
    """STEP 2 + STEP 3 of an S1 job in one ABI call: q = normalise(counts) (the all-reduced int64[S] vector), then the
    scores of the cached histograms H.  Returns (q, out32, out64)."""
    w = "combine_score_s1"
    pH, R = _rows(w + ": H", H, S)
    dev = H.device
    o32, o64, p64, p32 = _outs(w, R, S, dev, want32, want64, out32, out64)
    if q is None:
        q = torch.empty(S, dtype=torch.float32, device=dev)
    _ws, pws, nws = _scratch(w + ": ws", ws, dev, "epg_ws_bytes", 1, 0, N, S)
    _abi.call("epg_combine_score_s1", _arg(w + ": counts", counts, torch.int64, S, dev), 1 if rezero else 0, pH, R, N, S,
              _arg(w + ": q", q, torch.float32, S, dev), p64, p32, pws, nws, _stream())
    return q, o32, o64


def s1_tables(counts, N, S, q=None, ws=None):
    """STEP 2 and the S1 score table of group width N in ONE launch, nothing else (epg_combine_score_s1 with no bins):
    q = normalise(counts) and T[c, s] = kl(c / N, q[s]), c = 0..N.  Returns (q, T64, T32); the tables are views of `ws`."""
    pcounts, dev = _arg("s1_tables: counts", counts, torch.int64, S), counts.device
    if q is None:
        q = torch.empty(S, dtype=torch.float32, device=dev)
    ws, pws, nws = _scratch("s1_tables: ws", ws, dev, "epg_ws_bytes", 1, 0, N, S)
    _abi.call("epg_combine_score_s1", pcounts, 0, None, 0, N, S, _arg("s1_tables: q", q, torch.float32, S, dev), None, None, pws, nws, _stream())
    nent = (N + 1) * S
    off = (nent * 8 + 255) // 256 * 256
    return q, ws[:nent * 8].view(torch.float64), ws[off:off + nent * 4].view(torch.float32)


def score_s2(X, N, S, q, perms=None, want32=True, want64=False):
    pX, R, ldx = _mat("score_s2: X", X, torch.int8, N)
    dev = X.device
    perms = N * (N - 1) if perms is None else perms
    o32, o64, p64, p32 = _outs("score_s2", R, S, dev, want32, want64)
    _ws, pws, nws = _scratch("score_s2: ws", None, dev, "epg_ws_bytes", 2, R, N, S)
    _abi.call("epg_score_s2", pX, R, N, ldx, S, perms, _arg("score_s2: q", q, torch.float32, S * S, dev), p64, p32, pws, nws, _stream())
    return o32, o64


def score_s2_from_binhist(H, N, S, q, perms=None, want32=True, want64=False, out32=None, out64=None, ws=None):
    w = "score_s2_from_binhist"
    pH, R = _rows(w + ": H", H, S)
    dev = H.device
    perms = N * (N - 1) if perms is None else perms
    o32, o64, p64, p32 = _outs(w, R, S, dev, want32, want64, out32, out64)
    _ws, pws, nws = _scratch(w + ": ws", ws, dev, "epg_ws_bytes", 2, 0, N, S)
    _abi.call("epg_score_s2_from_binhist", pH, R, N, S, perms, _arg(w + ": q", q, torch.float32, S * S, dev), p64, p32, pws, nws, _stream())
    return o32, o64


def score_s3(X, N, S, q, want32=True, want64=False, ws=None):
    """`ws`: caller-owned workspace of at least epg_ws_bytes(3, R, N, S) bytes (tables + transposed matrix + cells)."""
    pX, R, ldx = _mat("score_s3: X", X, torch.int8, N)
    dev = X.device
    o32, o64, p64, p32 = _outs("score_s3", R, S, dev, want32, want64)
    _ws, pws, nws = _scratch("score_s3: ws", ws, dev, "epg_ws_bytes", 3, R, N, S)
    _abi.call("epg_score_s3", pX, R, N, ldx, S, _arg("score_s3: q", q, torch.float32, N * N * S * S, dev), p64, p32, pws, nws, _stream())
    return o32, o64


def _pair_tables(w, S, widths, tables, dev):
    """The four S1 tables of a paired call, float32 [width + 1, S] each -> their addresses."""
    return [_arg("%s: %s" % (w, name), T, torch.float32, (width + 1) * S, dev) for name, width, T in zip(("TA", "TB", "TnA", "TnB"), widths, tables)]


def pair_scores_s1_from_binhist(HA, HB, HnA, HnB, S, NA, NB, ga, gb, TA, TB, TnA, TnB):
    """Paired S1 in one pass over the four histograms (epg_pair_scores_s1_from_binhist): delta [R, S], null distance [R], STEP 4's
    distance [R] and 1-based largest-difference state [R].  T*: float32 [width + 1, S] device tables (scores.s1ScoreTable).
    Raises EpilogosHipError(-2) when the tables do not fit a CU's LDS; the separate calls give the same results."""
    w = "pair_scores_s1_from_binhist"
    pHA, R = _rows(w + ": HA", HA, S)
    dev = HA.device
    hists = [pHA] + [_arg("%s: %s" % (w, name), H, torch.int16, R * S, dev) for name, H in (("HB", HB), ("HnA", HnA), ("HnB", HnB))]
    delta = torch.empty((R, S), dtype=torch.float32, device=dev)
    null = torch.empty(R, dtype=torch.float32, device=dev)
    dist = torch.empty(R, dtype=torch.float32, device=dev)
    maxdiff = torch.empty(R, dtype=torch.int32, device=dev)
    _abi.call("epg_pair_scores_s1_from_binhist", *hists, R, S, NA, NB, ga, gb, *_pair_tables(w, S, (NA, NB, ga, gb), (TA, TB, TnA, TnB), dev),
              _ptr(delta), _ptr(null), _ptr(dist), _ptr(maxdiff), _stream())
    return delta, null, dist, maxdiff


def pair_scores_s1_parts(parts, S, NA, NB, ga, gb, TA, TB, TnA, TnB, qstate=None):
    """epg_pair_scores_s1_parts: `parts` is a list of (HA, HB, HnA, HnB) of the parts' histograms; one launch (per 24 parts) gives
    every part's delta [R, S], null distance [R], STEP 4's distance [R] and largest-difference state [R] and -- with qstate not
    None -- its quiescence mask uint8 [R] (qstate < 0: all zero).  Returns a list of dicts like _HipPairedSession._separate."""
    n = len(parts)
    if n == 0:
        return []
    w = "pair_scores_s1_parts"
    dev = parts[0][0].device
    rows = [p[0].shape[0] for p in parts]
    hists = [_parts("%s: parts[.][%d]" % (w, k), [p[k] for p in parts], torch.int16, [r * S for r in rows], dev) for k in range(4)]
    outs = []
    for R in rows:
        outs.append({"delta": torch.empty((R, S), dtype=torch.float32, device=dev), "null": torch.empty(R, dtype=torch.float32, device=dev),
                     "rdist": torch.empty(R, dtype=torch.float32, device=dev), "mdiff": torch.empty(R, dtype=torch.int32, device=dev),
                     "quies": torch.empty(R, dtype=torch.uint8, device=dev) if qstate is not None else None})
    out = lambda key: _ptr_array([o[key] for o in outs])
    _abi.call("epg_pair_scores_s1_parts", n, *hists, _ints(C.c_int64, rows), S, NA, NB, ga, gb,
              *_pair_tables(w, S, (NA, NB, ga, gb), (TA, TB, TnA, TnB), dev), out("delta"), out("null"), out("rdist"), out("mdiff"),
              out("quies") if qstate is not None else None, -1 if qstate is None else int(qstate), _stream())
    return outs


def _grid(where, x, dtype=torch.int32):
    """_arg for a dense [R, S] grid whose shape is the call's -> (address, R, S)."""
    p = _arg(where, x, dtype, 0)
    if x.dim() != 2:
        raise ValueError("engine.%s must be 2-D [R, S]" % where)
    return p, x.shape[0], x.shape[1]


def pair_finish(a, b, want_dist=True):
    pa, R, S = _grid("pair_finish: a", a, torch.float32)
    pb = _arg("pair_finish: b", b, torch.float32, R * S, a.device)
    delta = torch.empty_like(a)
    dist = torch.empty(R, dtype=torch.float32, device=a.device) if want_dist else None
    _abi.call("epg_pair_finish", pa, pb, R, S, _ptr(delta), _ptr(dist), _stream())
    return delta, dist


def pair_metrics(delta, roundtrip=True):
    """Signed squared distance float32[R] and 1-based largest-|delta| state int32[R] (roiAndVisualPairwise.py:347-354)."""
    pdelta, R, S = _grid("pair_metrics: delta", delta, torch.float32)
    dist = torch.empty(R, dtype=torch.float32, device=delta.device)
    maxdiff = torch.empty(R, dtype=torch.int32, device=delta.device)
    _abi.call("epg_pair_metrics", pdelta, R, S, 1 if roundtrip else 0, _ptr(dist), _ptr(maxdiff), _stream())
    return dist, maxdiff


def quiescent(XA, NA, XB, NB, qstate):
    pXA, R, ldxa = _mat("quiescent: XA", XA, torch.int8, NA)
    pXB, R2, ldxb = _mat("quiescent: XB", XB, torch.int8, NB, XA.device)
    if R != R2:
        raise ValueError("paired inputs must have the same number of bins")
    mask = torch.empty(R, dtype=torch.uint8, device=XA.device)
    _abi.call("epg_quiescent", pXA, NA, ldxa, pXB, NB, ldxb, R, qstate, _ptr(mask), _stream())
    return mask


def null_hist(XA, NA, XB, NB, S, ga, gb, seed, row0=0):
    pXA, R, ldxa = _mat("null_hist: XA", XA, torch.int8, NA)
    pXB, R2, ldxb = _mat("null_hist: XB", XB, torch.int8, NB, XA.device)
    if R != R2:
        raise ValueError("paired inputs must have the same number of bins")
    HA = torch.empty((R, S), dtype=torch.int16, device=XA.device)
    HB = torch.empty((R, S), dtype=torch.int16, device=XA.device)
    _abi.call("epg_null_hist", pXA, NA, ldxa, pXB, NB, ldxb, R, S, ga, gb, seed, row0, _ptr(HA), _ptr(HB), _stream())
    return HA, HB


_hip_rt = None


def _pinned_bytes(nbytes):
    """A page-locked int8 host tensor of EXACTLY nbytes, from hipHostMalloc through ctypes.  torch.empty(pin_memory=True) rounds
    every request up to a power of two (its caching host allocator): the 1.11 GB staging buffers of a whole-genome run became
    2 GiB each -- twice the memory to lock (0.15-0.6 s per buffer, during which every thread of the process that faults a page
    stands still) and to give back at exit.  torch recognises the memory as pinned (it asks the driver), so copies from it are
    asynchronous.  The buffers live as long as the process."""
    global _hip_rt
    if _hip_rt is None:
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                _hip_rt = C.CDLL(name)
                break
            except OSError:
                continue
        if _hip_rt is None:
            _hip_rt = False
    if _hip_rt:
        import weakref
        ptr = C.c_void_p()
        if _hip_rt.hipHostMalloc(C.byref(ptr), C.c_size_t(int(nbytes)), C.c_uint(0)) == 0 and ptr.value:
            # numpy array -> ctypes array (its base) -> the page-locked memory; the memory goes back to the driver when the last
            # of them -- i.e. the last tensor or view made from it -- is gone (a process that runs several jobs must not keep
            # 9 GB of page-locked memory per job)
            base = (C.c_int8 * int(nbytes)).from_address(ptr.value)
            weakref.finalize(base, _hip_rt.hipHostFree, C.c_void_p(ptr.value))
            t = torch.from_numpy(np.frombuffer(base, dtype=np.int8))
            if t.is_pinned():
                return t
            del t                                        # (the finalizer frees it)
    return torch.empty(int(nbytes), dtype=torch.int8, pin_memory=True)


class PinnedPool:
    """A few page-locked host staging buffers.  in_order=True hands them out IN TICKET ORDER (ticket k waits until tickets
    < k were served and a buffer is free): for a consumer that takes the parts in ticket order, parser threads running
    ahead can neither exhaust the pool nor starve the part it waits for.  in_order=False serves whoever asks first -- for a
    consumer that takes the parts as they complete (driver._stream_parts).  Buffers grow to the largest request and are
    reused for the whole run."""

    def __init__(self, n_buffers=3, in_order=True):
        import threading
        self.cv = threading.Condition()
        self.free = [None] * n_buffers          # None = not allocated yet
        self.next = 0
        self.in_order = in_order
        self.aborted = False
        self.weights = {}
        self.target = 0
        self.waiting = set()
        self.closed = False

    def hint(self, weights):
        """{ticket: bytes of the input file behind it}.  Page-locking memory is slow (~3 GB/s): a pool whose buffers grow to each
        larger request re-allocated ~1 GB a dozen times while the files of a genome completed smallest first (profiles/r04h:
        1.5 s between the end of chr1's parse and its hand-over).  With the hint, the first request scales its own size by
        (largest file / its file) and every buffer is allocated ONCE, at that size (+ 5 %)."""
        self.weights = dict(weights)

    def abort(self):
        """The consumer gave up (an error): wake every waiting parser thread instead of leaving it blocked."""
        with self.cv:
            self.aborted = True
            self.cv.notify_all()

    def acquire(self, ticket, nbytes):
        import os, sys, time
        trace = os.environ.get("EPILOGOS_TIMING") == "2"
        t_in = time.perf_counter()
        with self.cv:
            # among the readers waiting for a buffer the one with the LARGEST file goes first: the largest files finish last
            # and nothing can start behind them -- they are the critical path of the parse stage
            self.waiting.add(ticket)
            first = lambda: not self.weights or self.weights.get(ticket, 0) >= max(self.weights.get(t, 0) for t in self.waiting)
            self.cv.wait_for(lambda: self.aborted or ((not self.in_order or self.next == ticket) and len(self.free) > 0 and first()))
            self.waiting.discard(ticket)
            if self.aborted:
                raise RuntimeError("staging pool aborted")
            buf = self.free.pop()
            self.next += 1
            self.cv.notify_all()
        w = self.weights.get(ticket)
        if w and nbytes:
            self.target = max(self.target, int(nbytes / w * max(self.weights.values()) * 1.05))
        t_got = time.perf_counter()
        grew = 0
        if buf is None or buf.numel() < nbytes:
            buf = None                                   # (give the smaller buffer back before asking for the larger one)
            buf = _pinned_bytes(max(int(nbytes), self.target, 1 << 20))
            grew = buf.numel()
        if trace:
            print("    [pool] ticket %2d: waited %.2f s for a staging buffer%s  (at %.3f)" % (
                ticket, t_got - t_in, ", page-locked %.2f GB in %.2f s" % (grew / 1e9, time.perf_counter() - t_got) if grew else "",
                time.perf_counter()), file=sys.stderr, flush=True)
        return buf

    def skip(self, ticket):
        """A part that failed before asking for its buffer must not block the tickets behind it."""
        if not self.in_order:
            return
        with self.cv:
            self.cv.wait_for(lambda: self.aborted or self.next >= ticket)
            if self.next == ticket:
                self.next += 1
            self.cv.notify_all()

    def release(self, buf):
        with self.cv:
            if self.closed:
                return                                   # (dropped: the memory goes back to the driver with this last reference)
            self.free.append(buf)
            self.cv.notify_all()

    def close(self, background=True):
        """Nothing more will be staged: give the page-locked buffers back now -- on a helper thread, so that un-locking ~9 GB
        passes under the score pass and the writers instead of at process exit (0.3-0.4 s of a whole-genome run).  Buffers still
        out with an upload in flight are dropped when they come back."""
        import threading
        with self.cv:
            self.closed = True
            bufs, self.free = [b for b in self.free if b is not None], []
        if not bufs:
            return

        def work(bufs=bufs):
            while bufs:
                bufs.pop()
        if background:
            threading.Thread(target=work, name="epilogos-staging-close", daemon=True).start()
        else:
            work()


def upload_states(pinned, R, ldx, copy_stream, device="cuda"):
    """Asynchronous H2D copy of a staged [R, ldx] int8 matrix on `copy_stream`.  Returns (X, event): the current stream
    must wait for the event before reading X; the staging buffer may be reused once the event has completed.  X is allocated
    on the copy stream (the caching allocator then knows the copy may start at once) and recorded for the current stream,
    which is where the kernels that read it run."""
    with torch.cuda.stream(copy_stream):
        X = torch.empty((R, ldx), dtype=torch.int8, device=device)
        if R:
            X.copy_(pinned[:R * ldx].view(R, ldx), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(copy_stream)
    X.record_stream(torch.cuda.current_stream())
    return X, ev


def quiescent_from_binhist(HA, NA, HB, NB, S, qstate):
    """Quiescence mask from the two groups' histograms (scores.py:294-303)."""
    pHA, R = _rows("quiescent_from_binhist: HA", HA, S)
    pHB = _arg("quiescent_from_binhist: HB", HB, torch.int16, R * S, HA.device)
    mask = torch.empty(R, dtype=torch.uint8, device=HA.device)
    _abi.call("epg_quiescent_from_binhist", pHA, pHB, R, S, NA, NB, qstate, _ptr(mask), _stream())
    return mask


def null_hist_from_binhist(HA, HB, n_cols, S, ga, gb, seed, row0=0, stream=None):
    """Histograms of the two shuffled null groups from the REAL groups' histograms (multivariate hypergeometric, exact).
    stream: a torch.cuda.Stream to launch on instead of the current one (the outputs are allocated from the CURRENT stream's
    pool all the same; the caller orders the streams with events)."""
    pHA, R = _rows("null_hist_from_binhist: HA", HA, S)
    pHB = _arg("null_hist_from_binhist: HB", HB, torch.int16, R * S, HA.device)
    if HA.shape != HB.shape:
        raise ValueError("paired histograms must have the same shape")
    OA, OB = torch.empty_like(HA), torch.empty_like(HB)
    _abi.call("epg_null_hist_from_binhist", pHA, pHB, R, S, n_cols, ga, gb, seed, row0, _ptr(OA), _ptr(OB), _stream(stream))
    return OA, OB


def hist_to_numpy(H):
    """int16-stored uint16 histogram tensor -> numpy uint16."""
    return H.cpu().numpy().view(np.uint16)


# ---- similarity search (include/epilogos_amd.h, include/epilogos_simsearch_pick.h) and the scores-text parser
def simsearch_ws_bytes(Pg, S, W, B):
    return _scratch_bytes("epg_simsearch_ws_bytes", Pg, S, W, B, floor=0)


def simsearch(g, W, q, self_start, n, key_bound, ws=None, want_dist=False):
    """STEP 2's search (epg_simsearch): g int32 [Pg, S], q int32 [B, W, S], self_start int32 [B] -> (idx int32 [B, n], mode int64 [B],
    dist int64 [B, Pg - W + 1] or None), device tensors."""
    pg, Pg, S = _grid("simsearch: g", g)
    dev, B = g.device, int(self_start.numel()) if isinstance(self_start, torch.Tensor) else 0
    pq = _arg("simsearch: q", q, torch.int32, B * W * S, dev)
    pss = _arg("simsearch: self_start", self_start, torch.int32, B, dev)
    _ws, pws, nws = _scratch("simsearch: ws", ws, dev, "epg_simsearch_ws_bytes", Pg, S, W, B)
    idx = torch.empty((B, n), dtype=torch.int32, device=dev)
    mode = torch.empty(B, dtype=torch.int64, device=dev)
    dist = torch.empty((B, Pg - W + 1), dtype=torch.int64, device=dev) if want_dist else None
    _abi.call("epg_simsearch", pg, Pg, S, W, pq, B, pss, n, C.c_uint64(key_bound), pws, nws, _ptr(idx), _ptr(mode), _ptr(dist), _stream())
    return idx, mode, dist


def simsearch_reduce(x, blockSize):
    """The block-reduced genome (epg_simsearch_reduce): x int32 [R, S] -> int32 [ceil(R / blockSize), S]."""
    px, R, S = _grid("simsearch_reduce: x", x)
    g = torch.empty((-(-R // int(blockSize)), S), dtype=torch.int32, device=x.device)
    _abi.call("epg_simsearch_reduce", px, R, S, int(blockSize), _ptr(g), None, _stream())
    return g


def simsearch_slices(x, first, nblk, blockSize):
    """The block-reduced windows of x int32 [R, S] that start at rows `first` (a HOST int64 array, as the ABI wants) -> int32
    [B, nblk, S] (epg_simsearch_slices)."""
    px, R, S = _grid("simsearch_slices: x", x)
    first = np.ascontiguousarray(first, dtype=np.int64)
    q = torch.empty((len(first), int(nblk), S), dtype=torch.int32, device=x.device)
    _abi.call("epg_simsearch_slices", px, R, S, int(blockSize), int(nblk), first.ctypes.data_as(C.c_void_p), len(first), _ptr(q), _stream())
    return q


def simsearch_rowscore(x):
    """x int32 [G, S] -> float64 [G], pandas' row sums of the scores (epg_simsearch_rowscore)."""
    px, G, S = _grid("simsearch_rowscore: x", x)
    score = torch.empty(G, dtype=torch.float64, device=x.device)
    _abi.call("epg_simsearch_rowscore", px, G, S, _ptr(score), _stream())
    return score


def simsearch_rolling_max(v, W):
    """float64 [n] (contiguous) -> float64 [n], the centred rolling maximum (epg_simsearch_rolling_max)."""
    pv = _arg("simsearch_rolling_max: v", v, torch.float64, 0)
    out = torch.empty_like(v)
    _abi.call("epg_simsearch_rolling_max", pv, v.numel(), int(W), _ptr(out), _stream())
    return out


def simsearch_rank(rmax, rmean, score):
    """-> int32 [n] (the bits of the library's uint32): each window's position in np.lexsort((-score, -rmean, -rmax)) (epg_simsearch_rank)."""
    prmax, dev = _arg("simsearch_rank: rmax", rmax, torch.float64, 0), rmax.device
    n = rmax.numel()
    prmean, pscore = _arg("simsearch_rank: rmean", rmean, torch.float64, n, dev), _arg("simsearch_rank: score", score, torch.float64, n, dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    _ws, pws, nws = _scratch("simsearch_rank: ws", None, dev, "epg_simsearch_rank_ws_bytes", n)
    _abi.call("epg_simsearch_rank", prmax, prmean, pscore, n, _ptr(rank), pws, nws, _stream())
    return rank


def simsearch_pick(rank, W, maxRegions):
    """The greedy pick (epg_simsearch_pick): rank int32 [n] -> (picked int64 [ceil(n / W)], count int64 [1], device tensors; the
    sweeps over the tiles, a host int).  Synchronises as the header says."""
    prank, dev = _arg("simsearch_pick: rank", rank, torch.int32, 0), rank.device
    n = rank.numel()
    picked = torch.empty(max(-(-n // int(W)), 1), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    launches = C.c_int32(0)
    _ws, pws, nws = _scratch("simsearch_pick: ws", None, dev, "epg_simsearch_pick_ws_bytes", n, int(W))
    _abi.call("epg_simsearch_pick", prank, n, int(W), int(maxRegions), _ptr(picked), _ptr(count), C.byref(launches), pws, nws, _stream())
    return picked, count, int(launches.value)


def scores_ws_bytes(nbytes):
    return _scratch_bytes("epgt_scores_ws_bytes", nbytes, floor=0)


def scores_parse(text, nbytes, F, rows, row0, x, start, end, chrom_at, ws, status):
    """One chunk of a scores file parsed (epgt_scores_parse, include/epilogos_scores_text.h): text uint8 holds the chunk's nbytes
    bytes; rows row0 .. row0 + rows of x int32 [R, F - 3], start / end int64 [R] and chrom_at int32 [R] are written, status int64 [2]
    is the word all chunks share.  ws: scores_ws_bytes(nbytes) bytes at least."""
    w, top = "scores_parse: ", int(row0) + int(rows)
    ptext, dev = _arg(w + "text", text, torch.uint8, int(nbytes)), text.device
    _ws, pws, nws = _scratch(w + "ws", ws, dev, "epgt_scores_ws_bytes", int(nbytes))
    _abi.call("epgt_scores_parse", ptext, int(nbytes), int(F), int(rows), int(row0), _arg(w + "x", x, torch.int32, top * (int(F) - 3), dev),
              _arg(w + "start", start, torch.int64, top, dev), _arg(w + "end", end, torch.int64, top, dev),
              _arg(w + "chrom_at", chrom_at, torch.int32, top, dev), pws, nws, _arg(w + "status", status, torch.int64, 2, dev), _stream())
