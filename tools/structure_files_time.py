#!/usr/bin/env python3
"""Time align_from_structure_files phase by phase, and the structure front end alone.

    python tools/structure_files_time.py pipeline --num 128 --length 300 [--full | --fast]
    python tools/structure_files_time.py front --num 16384 --length 600 [--reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/structure_files_time.py front ...

pipeline: a synthetic ragged family (synthetic.make_ragged_family, lengths 0.8 x --length .. --length) is written as PDB
files (N, CA, C, O per residue) into a temporary folder; the phases of align_from_structure_files then run one after
the other, each timed on its own: parse (cleaning into cleaned_pdb/ and reading the C-alpha traces), features
(cr_structure_features; with --fast together with the guide tree in one cr_structure_shapemer_distance_matrix call),
guide tree (--full: make_pairwise_matrix -> max - M), progressive (multiple_align: neighbor joining and the progressive
alignment) and writers (FASTA and superposed PDB files).  The whole call, timed once more end to end, follows.

front: --num random-walk C-alpha traces of --length residues.  Times (median of --reps, wall clock of the whole call:
upload, kernels, download) cr_structure_features, cr_structure_shapemer_distance_matrix with and without the tensors,
and helper.local_shape_descriptor plus the numpy shapemer rule on the same set.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402


def _t(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def pipeline(num, length, full, seed=2027):
    from caretta_amd import helper, structure_io, synthetic
    from caretta_amd import multiple_alignment as ma
    from caretta_amd.engine import default_context
    default_context()
    fam = synthetic.make_ragged_family(num, int(0.8 * length), length, seed=seed)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        synthetic.write_pdb_family(fam, tmp / "in")
        out = ma.OutputFiles.from_folder(tmp / "out")
        out.output_folder.mkdir()
        ms = {}
        files, ms["parse"] = _t(lambda: structure_io.parse_protein_files_and_clean(tmp / "in", out.cleaned_pdb_folder, 16))
        calphas, t = _t(lambda: [helper.read_calpha_pdb(f) for f in files])
        ms["parse"] += t
        coords = [x for x, _ in calphas]
        if full:
            (tensors, _), ms["features"] = _t(lambda: helper.structure_features(coords, helper.STANDIN_WIDTH))
        else:
            (dist, tensors, _), ms["features+guide_tree"] = _t(
                lambda: helper.structure_shapemer_distance_matrix(coords, helper.STANDIN_WIDTH, return_features=True))
        names = [structure_io.structure_stem(f) for f in files]
        msa = ma.MultipleAlignment([ma.Protein(n, t, x, s) for n, t, (x, s) in zip(names, tensors, calphas)])
        prm = dict(flexible=False, gamma_tensor=7., gamma_coords=0.03)
        if full:
            m, ms["guide_tree"] = _t(lambda: msa.make_pairwise_matrix(score_function_params=prm))
            dist = m.max() - m
        aln, ms["progressive"] = _t(lambda: msa.multiple_align(dist, 1.0, 0.01, 1.0, 1., prm, dict(flexible=False)))

        def writers():
            msa.write_alignment(out.fasta_file)
            ma.write_superposed_pdbs(out.cleaned_pdb_folder, aln, out.pdb_folder)
        _, ms["writers"] = _t(writers)
        _, ms["align_from_structure_files"] = _t(lambda: ma.align_from_structure_files(
            tmp / "in", full=full, output_folder=tmp / "again", num_threads=16, write_fasta=True, write_pdb=True,
            verbose=False))
    return {"mode": "pipeline", "num": num, "length": length, "full": full, "ms": {k: round(v, 2) for k, v in ms.items()}}


def front(num, length, reps, seed=2028):
    from caretta_amd import helper
    from caretta_amd.engine import default_context
    default_context()
    rng = np.random.default_rng(seed)
    coords = []
    for _ in range(num):
        steps = rng.normal(size=(length, 3))
        steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
        coords.append(np.cumsum(steps, axis=0))
    w = helper.STANDIN_WIDTH
    res = {}
    for name, fn in (("structure_features", lambda: helper.structure_features(coords, w)),
                     ("shapemer_distance_matrix", lambda: helper.structure_shapemer_distance_matrix(coords, w)),
                     ("shapemer_distance_matrix+features",
                      lambda: helper.structure_shapemer_distance_matrix(coords, w, return_features=True))):
        fn()                                  # warm-up: device blocks, staging buffers
        res[name] = round(statistics.median(_t(fn)[1] for _ in range(reps)), 2)

    def numpy_rule():
        bits = 1 << np.arange(w - 1, -1, -1)
        return [((t >= 0.5) * bits).sum(axis=1) for t in (helper.local_shape_descriptor(x, w) for x in coords)]
    res["numpy local_shape_descriptor + rule"] = round(_t(numpy_rule)[1], 2)
    return {"mode": "front", "num": num, "length": length, "width": w, "ms": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["pipeline", "front"])
    ap.add_argument("--num", type=int, default=128)
    ap.add_argument("--length", type=int, default=300)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--full", action="store_true", help="all-vs-all guide tree (pipeline)")
    g.add_argument("--fast", action="store_true", help="shapemer guide tree (pipeline; the default)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = pipeline(a.num, a.length, a.full) if a.mode == "pipeline" else front(a.num, a.length, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
