"""STEP 4 of a paired run -- p-values / z-scores, metrics and regions of interest.  Same signature and
output files as the reference's epilogos/roiAndVisualPairwise.py main (:20-172) except for the figures:

    pairwiseMetrics_{tag}.txt.gz      writeMetrics :520-573
    regionsOfInterest_{tag}.txt       createROITxt :646-723 (with -n) / createROINoSignificance :726-778
    significantLoci_{tag}.txt.gz      createSignificantLociTxt :576-643 (with -n)

and it removes temp_*.npz and exp_freq like the reference (:341-343, :169).  The Manhattan and diagnostic plots
(:781-1190, matplotlib) are visualisation and are not produced.

The per-bin reduction of readInData (:347-354) -- signed squared distance and largest-difference state of every bin --
runs on the GPU (epg_pair_metrics): the scoring pass leaves it in temp_pairMetrics_{tag}_{stem}.npz next to the other
temporaries; without that side-car (outputs written by the reference itself) pairwiseDelta_*.txt.gz is parsed like the
reference does and the parsed matrix goes through the same kernel.  The statistics stay on the host and call the same
scipy routines as the reference (gennorm fit :245-270, cdf :496-517, zscore :101); the Benjamini-Hochberg step restates
statsmodels.stats.multitest.multipletests(method="fdr_bh") (:93; statsmodels==0.13.2 in requirements.txt, absent from
this image): p_(i) / (i/n) on the ascending p-values, running minimum from the right, clipped at 1."""
import gzip
import warnings
from contextlib import closing
from itertools import repeat
from multiprocessing import Pool, cpu_count
from os import remove
from pathlib import Path
from sys import argv
from time import time

import numpy as np
import pandas as pd
import scipy.stats as st

from . import _io
from . import backend as _backend
from .helpers import getNumStates, strToBool
from .roiSingle import _maxMeanOn, _roiOptions, findSign, getStateNames, maxMean, orderChromosomes


def benjaminiHochberg(pvals):
    """fdr_bh adjusted p-values, statsmodels' formula (multitest.py fdrcorrection with method 'indep')."""
    pvals = np.asarray(pvals, dtype=np.float64)
    n = len(pvals)
    if n == 0:
        return pvals.copy()
    order = np.argsort(pvals)
    ecdf = np.arange(1, n + 1) / float(n)
    raw = pvals[order] / ecdf
    corrected = np.minimum.accumulate(raw[::-1])[::-1]
    corrected[corrected > 1] = 1
    out = np.empty_like(corrected)
    out[order] = corrected
    return out


def _ordered_concat(chunks):
    order = orderChromosomes(list(chunks))
    return order, np.concatenate([chunks[c] for c in order]) if order else np.zeros(0)


def readNull(nullFile, quiescenceFile):
    """(chrName, nullDistances), (chrName, quiescenceArr) of one chromosome (reference :224-242)."""
    z, zq = np.load(Path(nullFile)), np.load(Path(quiescenceFile))
    return (z["chrName"][0], z["nullDistances"]), (zq["chrName"][0], zq["quiescenceArr"])


def fitOnSubSample(nullDistances, samplingSize, rng=None):
    """One trial of the null fit (reference roiAndVisualPairwise.py:245-270): generalised-normal parameters fitted to at most
    `samplingSize` null distances drawn without replacement, and the negative log-likelihood of ALL null distances under
    them.  Plain arrays in their own dtype (the float32 the score stage stored: scipy's optimiser sees what the reference's
    sees), (beta, loc, scale) and a float out; every trial draws from fresh OS entropy unless a
    numpy Generator is passed (the reference reseeds the global generator per call, which forked workers need)."""
    values = np.asarray(nullDistances)
    if values.size > samplingSize:
        rng = np.random.default_rng() if rng is None else rng
        fitted_on = values[rng.choice(values.size, size=samplingSize, replace=False)]
    else:
        fitted_on = values
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        params = st.gennorm.fit(fitted_on)
        return params, st.gennorm.nnlf(params, values)


_FIT_DATA = None                                     # the null distances of the pool's parent: workers inherit them through fork


def _fitOnSharedData(samplingSize):
    return fitOnSubSample(_FIT_DATA, samplingSize)


def _fitOptions(fit, seed):
    """What _fitParams is handed beyond its five arguments: nothing for the host fit, which is called as it always was."""
    return {} if fit == "host" else dict(fit=fit, seed=seed)


def fitDistances(outputDirPath, numProcesses, numTrials, samplingSize, fit="host", seed=None):
    """Null distances of the non-quiescent bins in chromosome order, `numTrials` fits, the one with the median
    negative log-likelihood wins (reference :175-221)."""
    nulls, quies = {}, {}
    for nf, qf in zip(sorted(outputDirPath.glob("temp_nullDistances_*.npz")),
                      sorted(outputDirPath.glob("temp_quiescence_*.npz"))):
        (c, d), (cq, qa) = readNull(nf, qf)
        nulls[c], quies[cq] = d, qa
    _, distanceArrNull = _ordered_concat(nulls)
    _, quiescenceArr = _ordered_concat(quies)
    nonQuiescentIdx = np.where(np.invert(quiescenceArr.astype(bool)))[0]
    return _fitParams(distanceArrNull, quiescenceArr, numProcesses, numTrials, samplingSize, **_fitOptions(fit, seed)), distanceArrNull, nonQuiescentIdx


def empiricalPVals(exceed, pool):
    """p = (1 + exceed) / (1 + M) in float64: the empirical p-value of a real distance that `exceed` of the M pooled null
    distances reach (--null-draws K > 1: M = K x non-quiescent bins).  The smallest attainable value is 1 / (1 + M)."""
    return (1.0 + np.asarray(exceed, dtype=np.float64)) / (1.0 + float(pool))


def readInData(outputDirPath, numStates, backend=None):
    """locationArr int64 [R,3] (chromosome number, start, end), signed squared distances float32 [R], 1-based
    largest-difference state int32 [R] and {number: chromosome}, sorted by location (reference :273-356)."""
    return _readInData(outputDirPath, numStates, backend)[:4]


def _readInData(outputDirPath, numStates, backend=None):
    """readInData, and as a fifth value the empirical p-values of the bins in the same order when every file has its
    temp_nullExceed_* side-car (a run with more than one null draw per bin), else None."""
    be = backend if backend is not None else _backend.get()
    deltas = sorted(outputDirPath.glob("pairwiseDelta_*.txt.gz"))
    chunks, exceed = {}, {}
    for f in deltas:
        tail = f.name[len("pairwiseDelta_"):-len(".txt.gz")]
        side = outputDirPath / "temp_pairMetrics_{}.npz".format(tail)
        if side.exists():
            z = np.load(side)
            chrom = np.full(len(z["distances"]), z["chrName"][0], dtype=object)
            part = (chrom, z["starts"], z["ends"], z["distances"], z["maxDiff"])
        else:
            df = pd.read_table(f, header=None, sep="\t")
            diffArr = np.ascontiguousarray(df.iloc[:, 3:3 + numStates].to_numpy(dtype=np.float32))
            dist, maxdiff = be.pair_metrics(diffArr, roundtrip=False)
            part = (df.iloc[:, 0].to_numpy(dtype=object), df.iloc[:, 1].to_numpy(dtype=np.int64),
                    df.iloc[:, 2].to_numpy(dtype=np.int64), dist, maxdiff)
        chunks[f] = part
        exc = outputDirPath / "temp_nullExceed_{}.npz".format(tail)
        if exc.exists():
            z = np.load(exc)
            exceed[f] = (z["nullExceed"], int(z["nullPool"][0]))
    chrom = np.concatenate([c[0] for c in chunks.values()]) if chunks else np.zeros(0, dtype=object)
    chrOrder = orderChromosomes(pd.unique(chrom))
    number = {c: i + 1 for i, c in enumerate(chrOrder)}
    chrDict = {i + 1: c for i, c in enumerate(chrOrder)}
    chrNum = np.array([number[c] for c in chrom], dtype=np.int64)
    starts = np.concatenate([c[1] for c in chunks.values()]).astype(np.int64)
    ends = np.concatenate([c[2] for c in chunks.values()]).astype(np.int64)
    dist = np.concatenate([c[3] for c in chunks.values()]).astype(np.float32)
    maxdiff = np.concatenate([c[4] for c in chunks.values()]).astype(np.int32)
    order = np.lexsort((ends, starts, chrNum))                      # sort_values(by=[chr, binStart, binEnd]) :332
    locationArr = np.stack([chrNum[order], starts[order], ends[order]], axis=1)
    pvals = None
    if chunks and len(exceed) == len(chunks):
        pvals = empiricalPVals(np.concatenate([exceed[f][0] for f in chunks]), max(m for _e, m in exceed.values()))[order]
    for file in outputDirPath.glob("temp_*.npz"):
        remove(file)
    return locationArr, dist[order], maxdiff[order], chrDict, pvals


def _pvals_chunk(x, beta, loc, scale):
    below = np.where(x <= loc)[0]
    above = np.where(x > loc)[0]
    pvals = np.zeros(len(x))
    pvals[below] = 2 * st.gennorm.cdf(x[below], beta, loc=loc, scale=scale)
    pvals[above] = 2 * (1 - st.gennorm.cdf(x[above], beta, loc=loc, scale=scale))
    return pvals


def calculatePVals(distanceArrReal, beta, loc, scale, threads=0):
    """Two-sided p-value of every distance under the fitted gennorm (reference :496-517).  The reference's expression,
    evaluated on slices of the array in threads (scipy's special functions release the GIL; elementwise, so the values are
    the single-threaded ones): 15 M distances took a third of this stage."""
    x = np.asarray(distanceArrReal)
    n = len(x)
    if threads <= 0:
        try:
            import os
            threads = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            threads = cpu_count()
        threads = min(threads, 32)
    step = max(1 << 18, -(-n // max(threads, 1)))
    if n <= step:
        return _pvals_chunk(x, beta, loc, scale)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(lambda lo: _pvals_chunk(x[lo:lo + step], beta, loc, scale), range(0, n, step)))
    return np.concatenate(parts)


def writeMetrics(locationArr, chrDict, maxDiffArr, nameArr, distanceArrReal, outputDirPath, fileTag, pvalBool, pvals=(),
                 mhPvals=()):
    """pairwiseMetrics_{tag}.txt.gz: chr, start, end, state, |distance| %.5f, sign [, p %.5e, BH p %.5e]
    (reference :520-573), through the native multi-threaded writer (same decompressed bytes)."""
    outputDirPath.mkdir(parents=True, exist_ok=True)
    numbers = sorted(chrDict)
    index = np.zeros(max(numbers) + 1 if numbers else 1, dtype=np.int32)
    index[numbers] = np.arange(len(numbers), dtype=np.int32)
    _io.write_metrics(outputDirPath / "pairwiseMetrics_{}.txt.gz".format(fileTag), [chrDict[n] for n in numbers],
                      index[locationArr[:, 0]] if len(locationArr) else np.zeros(0, dtype=np.int32), locationArr[:, 1],
                      locationArr[:, 2], list(nameArr), maxDiffArr, distanceArrReal, pvals if pvalBool else None,
                      mhPvals if pvalBool else None)


METRICS_DEVICE_REFUSED = ("WARNING: [--metrics gpu] the device does not format this file (a p-value outside [0, 1] or not a number, a distance "
                          "that is not finite, a state or a chromosome outside its table, a negative coordinate); writing it with the host writer instead")


def writeMetricsDevice(locationArr, chrDict, maxDiffArr, nameArr, distanceArrReal, outputDirPath, fileTag, pvalBool, pvals=(), mhPvals=(),
                       devicePvals=None):
    """writeMetrics with the rows formatted and compressed on the device (engine.metrics_text_bgzf, csrc/epg_metrics_text.h): the same
    decompressed bytes, always as BGZF with one end-of-file block, whatever EPILOGOS_BGZF and EPILOGOS_GZIP_LEVEL say.  devicePvals:
    (p, adjusted p) as float64 device tensors in the rows' order, when the p-value stage left them there (--pvals gpu): they are
    formatted where they sit.  -> False, and nothing is written, when the device refuses the file (a flag of the kernel)."""
    from . import driver, engine
    engine.require_gpu()
    outputDirPath.mkdir(parents=True, exist_ok=True)
    numbers = sorted(chrDict)
    index = np.zeros(max(numbers) + 1 if numbers else 1, dtype=np.int32)
    index[numbers] = np.arange(len(numbers), dtype=np.int32)
    p, mh = (None, None) if not pvalBool else (devicePvals if devicePvals is not None else (pvals, mhPvals))
    pieces = engine.metrics_text_bgzf([chrDict[n] for n in numbers], index[locationArr[:, 0]] if len(locationArr) else np.zeros(0, dtype=np.int32),
                                      locationArr[:, 1], locationArr[:, 2], list(nameArr), maxDiffArr, distanceArrReal, p, mh)
    if pieces is None:
        return False
    driver.write_bgzf(outputDirPath / "pairwiseMetrics_{}.txt.gz".format(fileTag), pieces)
    return True


def _writeMetricsOn(metrics, devicePvals=None):
    """The metrics writer of `metrics` ("host" or "gpu"): writeMetrics, or writeMetricsDevice with writeMetrics behind its refusal."""
    if metrics == "host":
        return writeMetrics
    if metrics != "gpu":
        raise ValueError("metrics must be 'host' or 'gpu', not {!r}".format(metrics))

    def write(*args, **kwargs):
        if not writeMetricsDevice(*args, devicePvals=devicePvals, **kwargs):
            print(METRICS_DEVICE_REFUSED, flush=True)
            writeMetrics(*args, **kwargs)
    return write


def _stars_p(p):
    return "***" if p <= 0.01 else ("**" if p <= 0.05 else ("*" if p <= 0.1 else "."))


def _stars_z(z):
    return "***" if z >= 3 else ("**" if z >= 2 else ("*" if z >= 1 else "."))


def createSignificantLociTxt(filePath, locationArr, chrDict, distanceArr, maxDiffArr, nameArr, pvals, mhPvals):
    """Every bin with BH p <= 0.1 (reference :576-643); the three floats go through float32 like the reference's frame."""
    with gzip.open(filePath, "wt") as out:
        for i in np.where(mhPvals <= 0.1)[0]:
            score = float(np.float32(distanceArr[i]))
            p, mh = float(np.float32(pvals[i])), float(np.float32(mhPvals[i]))
            out.write("{}\t{}\t{}\t{}\t{:.5f}\t{}\t{:.5e}\t{:.5e}\t{}\n".format(
                chrDict[locationArr[i, 0]], locationArr[i, 1], locationArr[i, 2], nameArr[int(maxDiffArr[i]) - 1], abs(score),
                findSign(score), p, mh, _stars_p(mh)))


def _regions(locationArr, distanceArr, roiWidth, roi="host"):
    """Top-100 maxmean windows over |distance| and, per window, the index of its most different bin
    (reference :682-689 / :755-762 with helpers.generateROIIndicesArr :277-296).  roi="gpu": searched on the device
    (roiSingle.maxMeanDevice), the same windows."""
    W = int(roiWidth)
    absd = np.abs(distanceArr)
    search = maxMean if roi == "host" else _maxMeanOn(roi)
    chrom, w_start, w_end, _, centre = search(locationArr[:, 0], locationArr[:, 1], locationArr[:, 2], absd, W, 100)
    maxIndices = np.zeros(len(centre), dtype=np.int64)
    for k, c in enumerate(centre):
        lo = int(c) - W // 2
        hi = int(c) + W // 2 + (1 if W % 2 else 0)
        maxIndices[k] = lo + int(np.argmax(absd[lo:hi]))
    return chrom, w_start, w_end, maxIndices


def createROITxt(filePath, locationArr, chrDict, distanceArr, maxDiffArr, nameArr, pvals, mhPvals, roiWidth, roi="host"):
    """Regions whose most different bin is significant, best first, cut at the first non-significant one
    (reference :646-723)."""
    with open(filePath, "w") as out:
        chrom, w_start, w_end, maxIndices = _regions(locationArr, distanceArr, roiWidth, **_roiOptions(roi))
        nonSig = np.where(mhPvals[maxIndices] > 0.1)[0]
        n = int(nonSig.min()) if len(nonSig) else len(maxIndices)
        for k in range(n):
            i = maxIndices[k]
            score = float(np.float32(distanceArr[i]))
            p, mh = float(np.float32(pvals[i])), float(np.float32(mhPvals[i]))
            out.write("{}\t{}\t{}\t{}\t{:.5f}\t{}\t{:.5e}\t{:.5e}\t{}\n".format(
                chrDict[int(chrom[k])], int(w_start[k]), int(w_end[k]), nameArr[int(maxDiffArr[i]) - 1], abs(score),
                findSign(score), p, mh, _stars_p(mh)))


def createROINoSignificance(filePath, locationArr, chrDict, distanceArr, maxDiffArr, nameArr, zScores, roiWidth, roi="host"):
    """Top-100 regions with the z-score of their most different bin (reference :726-778)."""
    with open(filePath, "w") as out:
        chrom, w_start, w_end, maxIndices = _regions(locationArr, distanceArr, roiWidth, **_roiOptions(roi))
        for k in range(len(maxIndices)):
            i = maxIndices[k]
            score = float(np.float32(distanceArr[i]))
            z = float(np.float32(zScores[i]))
            out.write("{}\t{}\t{}\t{}\t{:.5f}\t{}\t{:.5f}\t{}\n".format(
                chrDict[int(chrom[k])], int(w_start[k]), int(w_end[k]), nameArr[int(maxDiffArr[i]) - 1], abs(score),
                findSign(score), z, _stars_z(z)))


def _stage(verbose, label):
    if verbose: print(label + "...", flush=True)
    else: print("    " + label + "\t", end="", flush=True)
    return time()


def _done(verbose, t0):
    import os
    if verbose:
        print("    Time:", time() - t0, flush=True)
    elif os.environ.get("EPILOGOS_TIMING"):
        print("\t[Done] %.2f s" % (time() - t0), flush=True)
    else:
        print("\t[Done]", flush=True)


def medianTrial(nnlf):
    """The trial whose negative log-likelihood is the median one: the lower median of a stable ascending sort (reference :216-221)."""
    nnlf = np.asarray(nnlf, dtype=np.float64)
    return int(np.argsort(nnlf, kind="stable")[int((len(nnlf) - 1) / 2)])


FIT_SEED_TAG = 0x666974                              # "fit": the sub-samples' stream of a run's seed, apart from the null shuffles'


def fitIndices(M, numTrials, samplingSize, seed):
    """The sub-samples of the device fit: int32 [numTrials, samplingSize], row t = trial t's indices into the M null distances,
    drawn without replacement, trial after trial, from default_rng([seed, FIT_SEED_TAG]); None when M <= samplingSize (every
    trial fits all of them).  seed None: fresh OS entropy."""
    if M <= samplingSize:
        return None
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, FIT_SEED_TAG])
    return np.stack([rng.choice(M, size=samplingSize, replace=False) for _ in range(numTrials)]).astype(np.int32)


def _fitParamsGpu(data, numTrials, samplingSize, seed):
    """The fit="gpu" branch of _fitParams: one upload, one fit call, one nnlf call (include/epilogos_gennorm.h), the median pick on
    the host.  -> (beta, loc, scale), or None when a trial's sub-sample was degenerate (flag 2) or there is nothing to fit."""
    import torch
    from . import engine
    engine.require_gpu()
    values = np.ascontiguousarray(data, dtype=np.float32)
    if values.size < 2:
        return None
    x = torch.from_numpy(values).cuda()
    idx = fitIndices(values.size, numTrials, samplingSize, seed)
    # M <= samplingSize: every trial fits the same values and has the same likelihood; one trial's work stands for all
    params, _fval, info = engine.gennorm_fit(x, None if idx is None else torch.from_numpy(idx).cuda())
    nnlf = engine.gennorm_nnlf(x, params)
    if bool((info[:, 1] == 2).any()):
        return None
    params, nnlf = params.cpu().numpy(), nnlf.cpu().numpy()
    return tuple(params[medianTrial(nnlf) if idx is not None else 0])


def _fitParams(distanceArrNull, quiescenceArr, numProcesses, numTrials, samplingSize, fit="host", seed=None):
    """Median-likelihood gennorm fit of the non-quiescent null distances (reference :196-221).  fit="gpu": the trials and their
    likelihoods on the device, the sub-samples seeded from `seed` (fitIndices); no pool is forked."""
    data = distanceArrNull[np.where(np.invert(quiescenceArr.astype(bool)))[0]]
    if fit == "gpu":
        params = _fitParamsGpu(data, numTrials, samplingSize, seed)
        if params is not None:
            return params
        print("WARNING: a sub-sample of the null distances is constant or holds a value that is not finite; fitting on the host instead",
              flush=True)
        numProcesses = 1                             # in this process: the caller did not stop its writer threads for a fork
    elif fit != "host":
        raise ValueError("fit must be 'host' or 'gpu', not {!r}".format(fit))
    if numProcesses > 1 and numTrials > 1:
        # the reference pickles the whole array into every one of the numTrials tasks (:206-208, 43 MB x 101 at genome scale);
        # forked workers already have it
        global _FIT_DATA
        import multiprocessing
        if multiprocessing.get_start_method(allow_none=True) in (None, "fork"):
            _FIT_DATA = data
            try:
                with closing(multiprocessing.get_context("fork").Pool(numProcesses)) as pool:
                    results = pool.map(_fitOnSharedData, [samplingSize] * numTrials)
                pool.join()
            finally:
                _FIT_DATA = None
        else:
            with closing(Pool(numProcesses)) as pool:
                results = pool.starmap(fitOnSubSample, zip(repeat(data, numTrials), repeat(samplingSize, numTrials)))
            pool.join()
    else:
        results = [fitOnSubSample(data, samplingSize) for _ in range(numTrials)]
    return tuple(results[medianTrial([r[1] for r in results])][0])


def _pvalOptions(pvals):
    """What STEP 4 passes on beyond what it always passed: nothing for the host's p-value stage."""
    return {} if pvals == "host" else dict(pvals=pvals)


def _metricsOptions(metrics):
    """As _pvalOptions: nothing for the host's metrics writer."""
    return {} if metrics == "host" else dict(metrics=metrics)


def _pvalsGpu(distanceArrReal, params, empirical, keep=None):
    """The pvals="gpu" branch of _finish (csrc/epg_pvals.h): one upload of the distances and the three parameters, the p-value kernel
    and the Benjamini-Hochberg adjustment back to back on the device, one download of p, the adjusted p and the flag words.
    empirical given (--null-draws K > 1): the p-values are the host's and only the adjustment runs on the device.
    -> (pvals, mhPvals), or None when a flag word is not zero: a p-value that is NaN (a NaN distance, unusable parameters) or
    negative, or an iteration that stopped at its cap.  keep: a list that gets (p, adjusted p) as they sit on the device, for the
    metrics writer of --metrics gpu."""
    import torch
    from . import engine
    engine.require_gpu()
    if empirical is not None:
        pvals = np.ascontiguousarray(empirical, dtype=np.float64)
        p, pflags = torch.from_numpy(pvals).cuda(), None
    else:
        x = torch.from_numpy(np.ascontiguousarray(distanceArrReal, dtype=np.float32)).cuda()
        theta = torch.from_numpy(np.array([params[0], params[-2], params[-1]], dtype=np.float64)).cuda()
        p, pflags = engine.gennorm_pvals(x, theta)
    adj, bflags = engine.bh_adjust(p)
    flags = (bflags if pflags is None else torch.cat([pflags, bflags])).cpu().numpy()
    if flags.any():
        return None
    if keep is not None:
        keep.append((p, adj))
    return (pvals if empirical is not None else p.cpu().numpy()), adj.cpu().numpy()


def _finish(params, locationArr, distanceArrReal, maxDiffArr, chrDict, stateInfo, outputDirPath, fileTag, pvalBool, roiWidth,
            expFreqPath, verbose, empirical=None, pvals="host", roi="host", metrics="host"):
    """Everything of main() after the inputs are in memory (reference :72-169 without the figures).  empirical: the bins'
    empirical p-values (empiricalPVals); they take the place of the fitted distribution's and `params` is not used.
    pvals="gpu": the p-values and their Benjamini-Hochberg adjustment on the device (_pvalsGpu), both under the first of the two
    stage labels; a non-zero flag sends the whole stage back to the host functions.  roi="gpu": the region search on the device
    (roiSingle.maxMeanDevice).  metrics="gpu": pairwiseMetrics formatted and compressed on the device (writeMetricsDevice), from the
    device's own p-values when pvals="gpu" left them there."""
    if pvals not in ("host", "gpu"):
        raise ValueError("pvals must be 'host' or 'gpu', not {!r}".format(pvals))
    onDevice = pvals == "gpu"                        # (below, `pvals` is the array of p-values, as it always was)
    stateNameList = getStateNames(stateInfo)
    roiPath = outputDirPath / "regionsOfInterest_{}.txt".format(fileTag)
    if pvalBool:
        t0 = _stage(verbose, "Calculating p-vals")
        device, kept = None, []
        if onDevice and len(distanceArrReal):
            device = _pvalsGpu(distanceArrReal, params, empirical, **(dict(keep=kept) if metrics == "gpu" else {}))
            if device is None:
                print("WARNING: a p-value is not a number or negative, or an iteration met its cap; computing the p-values on the host instead",
                      flush=True)
        if device is not None:
            pvals, mhPvals = device
        else:
            pvals = empirical if empirical is not None else calculatePVals(distanceArrReal, params[0], params[-2], params[-1])
        _done(verbose, t0)
        t0 = _stage(verbose, "Benjamini-Hochberg procedure")
        if device is None:
            mhPvals = benjaminiHochberg(pvals)
        _done(verbose, t0)
        t0 = _stage(verbose, "Writing metrics")
        _writeMetricsOn(metrics, kept[0] if kept else None)(locationArr, chrDict, maxDiffArr, stateNameList, distanceArrReal, outputDirPath, fileTag, True,
                                                           pvals=pvals, mhPvals=mhPvals)
        del kept
        _done(verbose, t0)
        t0 = _stage(verbose, "Regions of interest txt")
        createROITxt(roiPath, locationArr, chrDict, distanceArrReal, maxDiffArr, stateNameList, pvals, mhPvals, roiWidth, **_roiOptions(roi))
        _done(verbose, t0)
        t0 = _stage(verbose, "Significant loci txt")
        createSignificantLociTxt(outputDirPath / "significantLoci_{}.txt.gz".format(fileTag), locationArr, chrDict,
                                 distanceArrReal, maxDiffArr, stateNameList, pvals, mhPvals)
        _done(verbose, t0)
    else:
        t0 = _stage(verbose, "Z-Scores")
        zScores = np.abs(st.zscore(distanceArrReal))
        _done(verbose, t0)
        t0 = _stage(verbose, "Writing metrics")
        _writeMetricsOn(metrics)(locationArr, chrDict, maxDiffArr, stateNameList, distanceArrReal, outputDirPath, fileTag, False)
        _done(verbose, t0)
        t0 = _stage(verbose, "Regions of interest txt")
        createROINoSignificance(roiPath, locationArr, chrDict, distanceArrReal, maxDiffArr, stateNameList, zScores, roiWidth, **_roiOptions(roi))
        _done(verbose, t0)
    remove(Path(expFreqPath))


def _is_location_sorted(chrNum, starts, ends):
    """True when rows are already in non-decreasing (chromosome, start, end) order -- then the stable lexsort is the identity."""
    if len(chrNum) < 2:
        return True
    c0, c1, s0, s1 = chrNum[:-1], chrNum[1:], starts[:-1], starts[1:]
    up = (c1 > c0) | ((c1 == c0) & ((s1 > s0) | ((s1 == s0) & (ends[1:] >= ends[:-1]))))
    return bool(up.all())


def mainFromArrays(results, stateInfo, outputDir, fileTag, numProcesses, pvalBool, numTrials, samplingSize, expFreqPath,
                   roiWidth, verbose, fit="host", seed=None, pvals="host", roi="host", metrics="host"):
    """main() on the arrays driver.run_paired_groups hands back ({stem: dict(chrName, locations, nullDistances,
    quiescenceArr, distances, maxDiff)}) instead of the temp_*.npz / pairwiseDelta text round trip."""
    outputDirPath = Path(outputDir)
    if numProcesses == 0:
        numProcesses = cpu_count()
    byChr = {v["chrName"]: v for v in results.values()}
    chrOrder = orderChromosomes(list(byChr))
    cat = lambda key: np.concatenate([byChr[c][key] for c in chrOrder])
    params = empirical = None
    if pvalBool and byChr and all("nullExceed" in v for v in byChr.values()):
        # more than one null draw per bin: empirical p-values against the pooled null, no fit
        empirical = empiricalPVals(cat("nullExceed"), max(int(v["nullPool"]) for v in byChr.values()))
    elif pvalBool:
        t0 = _stage(verbose, "Fitting distances")
        params = _fitParams(cat("nullDistances"), cat("quiescenceArr"), numProcesses, numTrials, samplingSize, **_fitOptions(fit, seed))
        _done(verbose, t0)
    cols = [byChr[c]["locations"].columns() for c in chrOrder]
    chrNum = np.concatenate([np.full(len(c[1]), i + 1, dtype=np.int64) for i, c in enumerate(cols)])
    starts, ends = np.concatenate([c[1] for c in cols]), np.concatenate([c[2] for c in cols])
    chrDict = {i + 1: c for i, c in enumerate(chrOrder)}
    dist, maxdiff = cat("distances"), cat("maxDiff")
    if _is_location_sorted(chrNum, starts, ends):
        # the usual case -- every file lists its bins in genomic order --: the stable three-key sort of 15 M rows (reference :332,
        # half of this stage's time at genome scale) is the identity
        locationArr = np.stack([chrNum, starts, ends], axis=1)
    else:
        order = np.lexsort((ends, starts, chrNum))
        locationArr = np.stack([chrNum[order], starts[order], ends[order]], axis=1)
        dist, maxdiff = dist[order], maxdiff[order]
        empirical = empirical[order] if empirical is not None else None
    _finish(params, locationArr, dist, maxdiff, chrDict, stateInfo, outputDirPath, fileTag, pvalBool, roiWidth, expFreqPath, verbose,
            empirical=empirical, **_pvalOptions(pvals), **_roiOptions(roi), **_metricsOptions(metrics))


def main(group1Name, group2Name, stateInfo, outputDir, fileTag, numProcesses, pvalBool, diagnosticBool, numTrials,
         samplingSize, expFreqPath, roiWidth, verbose, backend=None, fit="host", seed=None, pvals="host", roi="host", metrics="host"):
    tTotal = time()
    outputDirPath = Path(outputDir)
    numStates = getNumStates(stateInfo)
    if numProcesses == 0:
        numProcesses = cpu_count()
    params = None
    # temp_nullExceed_* next to the other temporaries (a run with more than one null draw per bin): empirical p-values, no fit
    empiricalRun = pvalBool and any(outputDirPath.glob("temp_nullExceed_*.npz"))
    if pvalBool and not empiricalRun:
        t0 = _stage(verbose, "Fitting distances")
        params, _, _ = fitDistances(outputDirPath, numProcesses, numTrials, samplingSize, fit=fit, seed=seed)
        _done(verbose, t0)
    t0 = _stage(verbose, "Reading in files")
    locationArr, distanceArrReal, maxDiffArr, chrDict, empirical = _readInData(outputDirPath, numStates, backend)
    _done(verbose, t0)
    if empiricalRun and empirical is None:
        raise ValueError("temp_nullExceed_*.npz is missing for some of the pairwiseDelta files in {}".format(outputDirPath))
    _finish(params, locationArr, distanceArrReal, maxDiffArr, chrDict, stateInfo, outputDirPath, fileTag, pvalBool, roiWidth,
            expFreqPath, verbose, empirical=empirical if empiricalRun else None, **_pvalOptions(pvals), **_roiOptions(roi),
            **_metricsOptions(metrics))
    if verbose: print("Total Time:", time() - tTotal, flush=True)


if __name__ == "__main__":
    main(argv[1], argv[2], argv[3], argv[4], argv[5], int(argv[6]), strToBool(argv[7]), strToBool(argv[8]), int(argv[9]),
         int(argv[10]), argv[11], int(argv[12]), strToBool(argv[13]))
