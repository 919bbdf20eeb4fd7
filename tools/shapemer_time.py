#!/usr/bin/env python3
"""Time the fast guide tree: cr_shapemer_distance_matrix (shapemer index lists -> P x P Bray-Curtis distances).

    python tools/shapemer_time.py [--sizes 1024,4096,16384] [--k 1024] [--length 600] [--reps 5] [--forms 0,1,2,3]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/shapemer_time.py --reps 3
    python tools/shapemer_time.py --trace DIR

Workload: P synthetic proteins in 16 clades, index lists of about 2 x 300 shapemers (geometricus' k-mer and radius
shapemers per residue) over K = 2^10 bins.  For each packing form (CARETTA_SHAPEMER_FORM: 0 the library's choice,
1 u8 v_sad_u8, 2 u16 v_pk_min_u16 + v_dot2_u32_u16, 3 u32 v_sad_u32) the tool prints the wall time of
the whole call (upload, kernels, download of the P x P f64 matrix into a pre-allocated array), median of --reps.

--trace DIR reads the rocprofv3 kernel trace of such a run and prints the device time of k_braycurtis per (form, P)
and its VALU-issue fraction: the reduction instructions the tiles need (wave64 instructions; one per packed word and
pair of rows for u8 / u32, two for u16) over kernel time x the issue peak of 256 CUs x 4 SIMDs x one wave64
VALU instruction per 2 cycles x 2.4 GHz = 1.23e12 per second.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time
from collections import defaultdict
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402

TILE = 64
VALU_ISSUE_PEAK = 256 * 4 * 2.4e9 / 2
FORM_NAMES = {1: "u8 v_sad_u8", 2: "u16 v_pk_min_u16 + v_dot2", 3: "u32 v_sad_u32"}
BINS_PER_WORD = {1: 4, 2: 2, 3: 1}
OPS_PER_WORD = {1: 1, 2: 2, 3: 1}


def workload(num, k, length, seed=2026):
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, k, size=length) for _ in range(16)]
    lists = []
    for p in range(num):
        n = length + int(rng.integers(-length // 10, length // 10 + 1))
        lst = rng.choice(bases[p % 16], size=n)
        redraw = rng.random(n) < 0.3
        lst[redraw] = rng.integers(0, k, size=int(redraw.sum()))
        lists.append(lst)
    return lists


def reduction_instructions(num, k, form):
    tiles = -(-num // TILE)
    words = -(-k // 128) * 128 // BINS_PER_WORD[form]
    return tiles * (tiles + 1) // 2 * TILE * words * OPS_PER_WORD[form]


def time_calls(args):
    from caretta_amd import _capi, engine
    from caretta_amd.multiple_alignment import _index_lists
    ctx = engine.default_context()
    lib = _capi.load()
    out = []
    for num in args.sizes:
        idx, offsets = _index_lists(workload(num, args.k, args.length))
        d = np.empty((num, num))
        for form in args.forms:
            os.environ["CARETTA_SHAPEMER_FORM"] = str(form)
            engine.reload_config()
            times = []
            for rep in range(args.reps + 1):                   # the first call warms up
                t0 = time.perf_counter()
                _capi.check(lib.cr_shapemer_distance_matrix(ctx._h, _capi.ptr(idx), _capi.ptr(offsets), num, args.k,
                                                            _capi.ptr(d)))
                if rep:
                    times.append((time.perf_counter() - t0) * 1e3)
            rec = {"P": num, "K": args.k, "form": form, "call_ms_median": statistics.median(times),
                   "call_ms_min": min(times), "d_checksum": float(d.sum()), "d_max": float(d.max())}
            out.append(rec)
            print(f"P={num:6d} K={args.k} form {form} ({FORM_NAMES.get(form, 'library choice')}): whole call "
                  f"{rec['call_ms_median']:.3f} ms median ({rec['call_ms_min']:.3f} min) of {args.reps}; checksum {rec['d_checksum']:.6f}",
                  flush=True)
    os.environ.pop("CARETTA_SHAPEMER_FORM", None)
    engine.reload_config()
    if args.json:
        Path(args.json).write_text(json.dumps(out, indent=1))


def summarize_trace(root, k):
    per = defaultdict(list)
    for path in glob.glob(f"{root}/**/*kernel_trace.csv", recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                m = re.search(r"k_braycurtis<(\d)>", r["Kernel_Name"])
                if not m:
                    continue
                tiles = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
                per[(int(m.group(1)), tiles)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    if not per:
        sys.exit(f"no k_braycurtis dispatches under {root}")
    for (form, tiles), ms in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        num = tiles * TILE
        best = min(ms)
        frac = reduction_instructions(num, k, form) / (best * 1e-3) / VALU_ISSUE_PEAK
        pairs = num * (num + 1) / 2
        print(f"P<={num:6d} (tiles {tiles}) form {form} ({FORM_NAMES[form]}): k_braycurtis {best:.3f} ms min, "
              f"{statistics.median(ms):.3f} median of {len(ms)}; {pairs * k / (best * 1e-3) / 1e12:.2f} T bin-pairs/s; "
              f"VALU-issue fraction {frac:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", default="0,1,2,3")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", default=None, help="summarize a rocprofv3 --kernel-trace directory instead of timing")
    args = ap.parse_args()
    if args.trace:
        summarize_trace(args.trace, args.k)
        return
    args.sizes = [int(x) for x in args.sizes.split(",")]
    args.forms = [int(x) for x in args.forms.split(",")]
    time_calls(args)


if __name__ == "__main__":
    main()
