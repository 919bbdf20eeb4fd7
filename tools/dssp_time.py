"""Time the DSSP feature path (cr_dssp_features): host parsing and the device call, at the three kringles and at a
synthetic full-atom batch (default 16 384 structures of 600 residues, about 7.8 heavy atoms per residue).  The batch is
64 distinct synthetic chains repeated, so that building it stays quick; the device does the full work for every copy.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/dssp/README.md).

    python tools/dssp_time.py [--num 16384] [--length 600] [--reps 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num", type=int, default=16384)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    from caretta_amd import feature_extraction, structure_io, synthetic
    from caretta_amd.engine import default_context
    default_context()
    result = {}
    files = sorted((ROOT / "tests" / "golden" / "c1_pdb").glob("*.pdb"))
    t0 = time.perf_counter()
    parsed = [structure_io.read_dssp_atoms(f) for f in files]
    result["kringles_parse_ms"] = (time.perf_counter() - t0) * 1e3
    feature_extraction.dssp_features_batch(parsed)            # warm-up
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        feature_extraction.dssp_features_batch(parsed)
        times.append((time.perf_counter() - t0) * 1e3)
    result["kringles_device_call_ms"] = times
    base = synthetic.make_full_atom_family(min(64, args.num), args.length, args.length, seed=31)
    batch = [base[i % len(base)] for i in range(args.num)]
    result["batch"] = {"structures": args.num, "residues": args.num * args.length,
                       "atoms": int(sum(len(s.atoms) for s in batch))}
    feature_extraction.dssp_features_batch(batch[:64])        # warm-up
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        feature_extraction.dssp_features_batch(batch)
        times.append((time.perf_counter() - t0) * 1e3)
    result["batch_call_ms"] = times
    line = json.dumps(result)
    print(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
