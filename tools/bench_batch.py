#!/usr/bin/env python3
"""bench_batch.py — throughput of fv_decode_full_batch against a loop of fv_decode_full calls.

  python tools/bench_batch.py [--nseq 1 8 32 64] [--min-seconds 0.5] [--alternations 5] [--debug V]
                              [--out profiles/batch_full_bench.json] [--git-head REV]
  python tools/bench_batch.py --once NSEQ      # warm up, then ONE batch call (the run to put under rocprofv3)

One process, one context, the model of bench.py's default workload (K = 3965, M = 50, density 0.112, seed 12), T = 256,
n_split = 8, FV_MODE_REFERENCE, nseq distinct seeded sequences (sequence 0 is bench.py's own).  Per nseq, after both
variants are warm and their paths have been compared (exactly), two timings alternate:

  (a) loop    nseq consecutive fv_decode_full calls (the existing entry point)
  (b) batch   one fv_decode_full_batch call

Both through ctypes with preallocated buffers, a host clock around calls that end in the library's own synchronise, each
timing repeated until --min-seconds of timed work, --alternations times.  Reported per variant: median and range of
sequences/s and of cells/s (cells = K*K*T per sequence, bench.py's metric).  --debug V sets FV_OPT_DEBUG for the batch
calls only (bit 28: generation 0 on one stream).  --kernels: FV_KERNEL_* values to run (default 0 = the library's choice,
the walk over the non-zero transitions for this model, and 6 = the dense 16-bit kernel bench.py times).  The JSON goes to
--out and to stdout.

  python tools/bench_batch.py --beam B [--shape cfg2|cfg4] [--nseq 1 8 32] [--debug V] [--once NSEQ]

FLASH-BS: the same protocol with (a) a loop of fv_decode_beam calls and (b) one fv_decode_beam_batch call, beam width B,
on the model of the shape (cfg2: K = 3965, cfg4: K = 16384; T = 256, n_split = 8); cells = K*B*T per sequence.  Without
--debug both launch forms of generation 0 are timed (FV_OPT_DEBUG 0 and bit 29), each against the loop in the same
alternation.  Default --out: profiles/batch_beam_bench.json, one entry per shape (entries of other shapes are kept).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

K, T, M_SYMBOLS, PROB, SEED, N_SPLIT = 3965, 256, 50, 0.112, 12, 8
SHAPE_K = {"cfg2": 3965, "cfg4": 16384}


def git_head(given):
    if given:
        return given
    try:
        res = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, timeout=30)
        if res.returncode == 0:
            dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, timeout=30).stdout.strip()
            return res.stdout.strip() + ("+modified" if dirty else "")
    except (OSError, subprocess.SubprocessError):
        pass
    return "unknown (not a git checkout; pass --git-head)"


class Runner:
    def __init__(self, fv, obs, debug):
        self.fv, self.L, self.h, self.debug = fv, decoder.load_library(), fv._h, debug
        self.obs = obs
        self.n = len(obs)
        self.cat = np.ascontiguousarray(np.concatenate(obs), dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum([o.size for o in obs])]).astype(np.int64)
        self.loop_path = np.empty(self.cat.size, dtype=np.int32)
        self.batch_path = np.empty(self.cat.size, dtype=np.int32)
        self.loop_score = np.zeros(self.n, dtype=np.float32)
        self.batch_score = np.zeros(self.n, dtype=np.float32)
        self.status = np.zeros(self.n, dtype=np.int32)
        vp = ctypes.c_void_p
        self._loop_args = [(obs[s].ctypes.data_as(vp), obs[s].size, self.loop_path[self.offsets[s]:].ctypes.data_as(vp),
                            self.loop_score[s:].ctypes.data_as(vp)) for s in range(self.n)]
        self._batch_args = (self.cat.ctypes.data_as(vp), self.offsets.ctypes.data_as(vp), self.n, N_SPLIT, decoder.MODE_REFERENCE,
                            self.batch_path.ctypes.data_as(vp), self.batch_score.ctypes.data_as(vp), self.status.ctypes.data_as(vp))

    def loop(self):
        f, h = self.L.fv_decode_full, self.h
        for ob, n, path, score in self._loop_args:
            rc = f(h, ob, n, N_SPLIT, decoder.MODE_REFERENCE, path, score)
            if rc:
                raise decoder.FlashVitError(rc, "fv_decode_full in the loop")

    def batch(self):
        if self.debug:
            self.fv.set_option(decoder.OPT_DEBUG, self.debug)
        try:
            rc = self.L.fv_decode_full_batch(self.h, *self._batch_args)
        finally:
            if self.debug:
                self.fv.set_option(decoder.OPT_DEBUG, 0)
        if rc:
            raise decoder.FlashVitError(rc, self.L.fv_last_error_detail(self.h).decode())

    def check(self):
        self.batch_path[:] = -7
        self.loop()
        self.batch()
        assert self.loop_path.tolist() == self.batch_path.tolist(), "batch paths differ from the single calls'"
        assert (self.loop_score == self.batch_score).all() and not self.status.any()


def timed(fn, min_seconds):
    """seconds per call of fn, from repeated calls worth at least min_seconds"""
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / calls, calls


class BeamRunner(Runner):
    """loop of fv_decode_beam against one fv_decode_beam_batch (a beam miss is a result, not a failure)"""

    def __init__(self, fv, obs, debug, beam):
        super().__init__(fv, obs, debug)
        self.beam = beam
        self._batch_args = self._batch_args[:4] + (beam,) + self._batch_args[4:]

    def loop(self):
        f, h = self.L.fv_decode_beam, self.h
        for ob, n, path, score in self._loop_args:
            rc = f(h, ob, n, N_SPLIT, self.beam, decoder.MODE_REFERENCE, path, score)
            if rc < 0:
                raise decoder.FlashVitError(rc, "fv_decode_beam in the loop")

    def batch(self):
        self.fv.set_option(decoder.OPT_DEBUG, self.debug)
        try:
            rc = self.L.fv_decode_beam_batch(self.h, *self._batch_args)
        finally:
            self.fv.set_option(decoder.OPT_DEBUG, 0)
        if rc < 0:
            raise decoder.FlashVitError(rc, self.L.fv_last_error_detail(self.h).decode())

    def check(self):
        self.batch_path[:] = -7
        self.loop()
        self.batch()
        assert self.loop_path.tolist() == self.batch_path.tolist(), "batch paths differ from the single calls'"
        assert (self.loop_score == self.batch_score).all()


def main_beam(args):
    k = SHAPE_K[args.shape]
    A64, B64, Pi64 = data_script.make_model64(k, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    del A64
    rs = np.random.RandomState(SEED)
    most = max(args.nseq + [args.once])
    obs = [np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)]
    obs += [rs.randint(0, M_SYMBOLS, T).astype(np.int32) for _ in range(most - 1)]
    forms = [args.debug] if args.debug is not None else [0, decoder.DEBUG_BEAM_BATCH_GEN0_OTHER]
    cells = float(k) * args.beam * T
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    try:
        if args.once:
            r = BeamRunner(fv, obs[:args.once], forms[0], args.beam)
            r.check()
            r.batch()
            st = fv.stats()
            print(json.dumps(dict(once=args.once, beam=args.beam, shape=args.shape, debug=forms[0], gpu_ms=st["gpu_ms"], decode_ms=st["decode_ms"],
                                  step_launches=st["step_launches"], passes=st["passes"], generations=st["generations"],
                                  reach_events=st["beam_reach_events"], exact_sets=st["beam_exact_sets"], device_bytes=st["device_bytes"])))
            return
        entry = dict(shape=args.shape, git_head=git_head(args.git_head), K=k, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, n_split=N_SPLIT,
                     beam=args.beam, mode="reference", min_seconds=args.min_seconds, alternations=args.alternations, results=[])
        for nseq in args.nseq:
            runners = [BeamRunner(fv, obs[:nseq], d, args.beam) for d in forms]
            for r in runners:
                r.check()                              # warms both variants and compares their paths and scores
                r.check()
            loop_t, batch_t = [], [[] for _ in runners]
            for _ in range(args.alternations):
                loop_t.append(timed(runners[0].loop, args.min_seconds)[0])
                for r, bt in zip(runners, batch_t):
                    bt.append(timed(r.batch, args.min_seconds)[0])
            a = summary(loop_t, nseq, cells)
            for r, bt in zip(runners, batch_t):
                r.batch()
                st = fv.stats()
                b = summary(bt, nseq, cells)
                entry["results"].append(dict(nseq=nseq, batch_debug=r.debug, loop=a, batch=b, speedup_median=b["seq_per_s_median"] / a["seq_per_s_median"],
                                             beats_loop_by_more_than_both_ranges=b["seq_per_s_min"] - a["seq_per_s_max"] >
                                             (b["seq_per_s_max"] - b["seq_per_s_min"]) + (a["seq_per_s_max"] - a["seq_per_s_min"]),
                                             batch_gpu_ms=st["gpu_ms"], batch_step_launches=st["step_launches"], batch_passes=st["passes"],
                                             reach_events=st["beam_reach_events"], exact_sets=st["beam_exact_sets"], device_bytes=st["device_bytes"]))
                print(f"{args.shape} B {args.beam} nseq {nseq:3d} debug {r.debug}: loop {a['seq_per_s_median']:8.1f} seq/s ({a['seq_per_s_min']:.1f}-{a['seq_per_s_max']:.1f})  "
                      f"batch {b['seq_per_s_median']:8.1f} seq/s ({b['seq_per_s_min']:.1f}-{b['seq_per_s_max']:.1f})  "
                      f"x{entry['results'][-1]['speedup_median']:.2f}", file=sys.stderr, flush=True)
    finally:
        fv.close()
    path = args.out or os.path.join(ROOT, "profiles", "batch_beam_bench.json")
    out = dict(tool="tools/bench_batch.py --beam", shapes=[])
    if os.path.isfile(path):
        with open(path) as fh:
            old = json.load(fh)
        out["shapes"] = [e for e in old.get("shapes", []) if e.get("shape") != args.shape or e.get("beam") != args.beam]
    out["shapes"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(entry))


def summary(per_call, nseq, cells=float(K) * K * T):
    rate = sorted(nseq / t for t in per_call)
    return dict(seq_per_s_median=statistics.median(rate), seq_per_s_min=rate[0], seq_per_s_max=rate[-1],
                cells_per_s_median=statistics.median(rate) * cells, cells_per_s_min=rate[0] * cells, cells_per_s_max=rate[-1] * cells,
                ms_per_sequence_median=1e3 / statistics.median(rate), range_rel=(rate[-1] - rate[0]) / statistics.median(rate))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nseq", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--debug", type=int, default=None)
    ap.add_argument("--beam", type=int, default=0)
    ap.add_argument("--shape", choices=sorted(SHAPE_K), default="cfg2")
    ap.add_argument("--kernels", type=int, nargs="+", default=[decoder.KERNEL_AUTO, decoder.KERNEL_U16_REFINE])
    ap.add_argument("--out", default="")
    ap.add_argument("--git-head", default="")
    ap.add_argument("--once", type=int, default=0)
    args = ap.parse_args()
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    if args.beam:
        if args.nseq == [1, 8, 32, 64]:
            args.nseq = [1, 8, 32]
        return main_beam(args)
    args.debug = args.debug or 0
    args.out = args.out or os.path.join(ROOT, "profiles", "batch_full_bench.json")

    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    rs = np.random.RandomState(SEED)
    most = max(args.nseq + [args.once])
    obs = [np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)]
    obs += [rs.randint(0, M_SYMBOLS, T).astype(np.int32) for _ in range(most - 1)]
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, Pi)
    try:
        if args.once:
            fv.set_option(decoder.OPT_KERNEL, args.kernels[0])
            r = Runner(fv, obs[:args.once], args.debug)
            r.check()
            r.batch()
            st = fv.stats()
            print(json.dumps(dict(once=args.once, gpu_ms=st["gpu_ms"], decode_ms=st["decode_ms"], step_launches=st["step_launches"],
                                  passes=st["passes"], generations=st["generations"])))
            return
        out = dict(tool="tools/bench_batch.py", git_head=git_head(args.git_head), K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED,
                   n_split=N_SPLIT, mode="reference", batch_debug=args.debug, min_seconds=args.min_seconds,
                   alternations=args.alternations, results=[])
        for kernel, nseq in [(k, n) for k in args.kernels for n in args.nseq]:
            fv.set_option(decoder.OPT_KERNEL, kernel)
            r = Runner(fv, obs[:nseq], args.debug)
            r.check()                                  # warms both variants and compares their paths and scores
            r.check()
            loop_t, batch_t = [], []
            for _ in range(args.alternations):
                loop_t.append(timed(r.loop, args.min_seconds)[0])
                batch_t.append(timed(r.batch, args.min_seconds)[0])
            r.batch()
            st = fv.stats()
            a, b = summary(loop_t, nseq), summary(batch_t, nseq)
            out["results"].append(dict(kernel_option=kernel, kernel=st["kernel"], nseq=nseq, loop=a, batch=b, speedup_median=b["seq_per_s_median"] / a["seq_per_s_median"],
                                       batch_gpu_ms=st["gpu_ms"], batch_step_launches=st["step_launches"], batch_passes=st["passes"],
                                       device_bytes=st["device_bytes"]))
            print(f"kernel {st['kernel']} nseq {nseq:3d}: loop {a['seq_per_s_median']:8.1f} seq/s ({a['seq_per_s_min']:.1f}-{a['seq_per_s_max']:.1f})  "
                  f"batch {b['seq_per_s_median']:8.1f} seq/s ({b['seq_per_s_min']:.1f}-{b['seq_per_s_max']:.1f})  "
                  f"x{out['results'][-1]['speedup_median']:.2f}", file=sys.stderr, flush=True)
    finally:
        fv.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
