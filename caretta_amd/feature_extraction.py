"""DSSP features on the device: the reference's ``feature_extraction.get_features`` / ``get_features_multiple``
(feature_extraction.py:122-253) with ``only_dssp=True``, without mkdssp or ProDy.

The reference runs an external ``mkdssp`` through ProDy and reads its text.  Here the H-bond energies, secondary structure,
backbone angles and solvent accessibility are computed by ``cr_dssp_features`` (caretta_amd/csrc/cr_dssp.h) after Kabsch
& Sander (1983), with the choices written down in DESIGN section 4.6.  The results are NOT mkdssp's.  GNM / ANM
fluctuations and residue depth (``only_dssp=False``) are not available.

``python -m caretta_amd.feature_extraction RESULTS_FOLDER`` adds ``result_features.pkl`` to a finished
``align_from_structure_files`` results folder (``result.fasta`` and ``cleaned_pdb/``), as the reference's
``write_features`` does (multiple_alignment.py:549-560).
"""
from __future__ import annotations

import math
import pickle
import sys
import typing
from pathlib import Path

import numpy as np

from . import _capi, structure_io
from ._capi import check, ptr

# the keys, in the row order of cr_dssp_features' output, then "secondary"
DSSP_KEYS = ("dssp_NH_O_1_index", "dssp_NH_O_1_energy", "dssp_O_NH_1_index", "dssp_O_NH_1_energy",
             "dssp_NH_O_2_index", "dssp_NH_O_2_energy", "dssp_O_NH_2_index", "dssp_O_NH_2_energy",
             "dssp_acc", "dssp_alpha", "dssp_kappa", "dssp_phi", "dssp_psi", "dssp_tco")
INTEGER_KEYS = ("dssp_NH_O_1_index", "dssp_O_NH_1_index", "dssp_NH_O_2_index", "dssp_O_NH_2_index", "dssp_acc")
NUM_SPHERE_POINTS = 401

_NOT_AVAILABLE = ("only_dssp=False: GNM / ANM fluctuations (ProDy's normal-mode solvers) and residue depth (the external "
                  "MSMS program) are not available in caretta_amd; only the DSSP features are")


def sphere_points(n: int = NUM_SPHERE_POINTS) -> np.ndarray:
    """The golden-spiral point table of the accessibility, built once on the host in f64: for k = -(n-1)/2 .. (n-1)/2,
    lat = asin(2k / n), lon = fmod(k, phi) * 2 pi / phi, point (sin lon cos lat, cos lon cos lat, sin lat)."""
    golden = (1.0 + math.sqrt(5.0)) / 2.0
    half = (n - 1) // 2
    out = np.empty((n, 3), dtype=np.float64)
    for row, k in enumerate(range(-half, n - half)):
        lat = math.asin(2.0 * k / n)
        lon = math.fmod(k, golden) * 2.0 * math.pi / golden
        out[row] = (math.sin(lon) * math.cos(lat), math.cos(lon) * math.cos(lat), math.sin(lat))
    return out


RAW_ANGLE_KEYS = ("dssp_alpha", "dssp_kappa", "dssp_phi", "dssp_psi", "dssp_tco")


def dssp_features_batch(structures: typing.Sequence[structure_io.DsspAtoms], raw_angles: bool = False):
    """One device pass (cr_dssp_features) for every structure; one feature dict per structure, each value (L,).
    raw_angles: also return, per structure, {key: (L,)} of alpha / kappa / phi / psi / tco before rounding (0 where no
    residue maps), as (features, raw)."""
    if not structures:
        return ([], []) if raw_angles else []
    num = len(structures)
    res_off = np.zeros(num + 1, dtype=np.int64)
    ca_off = np.zeros(num + 1, dtype=np.int64)
    np.cumsum([len(s.is_pro) for s in structures], out=res_off[1:])
    np.cumsum([s.num_residues for s in structures], out=ca_off[1:])
    backbone = np.ascontiguousarray(np.concatenate([s.backbone.reshape(-1, 12) for s in structures]), dtype=np.float64)
    is_pro = np.ascontiguousarray(np.concatenate([s.is_pro for s in structures]), dtype=np.int32)
    atoms = np.ascontiguousarray(np.concatenate([s.atoms.reshape(-1, 3) for s in structures]), dtype=np.float64)
    classes = np.ascontiguousarray(np.concatenate([s.radius_class for s in structures]), dtype=np.int32)
    atom_off = np.zeros(int(res_off[-1]) + 1, dtype=np.int64)
    np.cumsum(np.concatenate([np.diff(s.atom_offsets) for s in structures]), out=atom_off[1:])
    points = sphere_points()
    total = int(ca_off[-1])
    out = np.empty((len(DSSP_KEYS), total), dtype=np.float64)
    codes = np.empty(total, dtype=np.uint8)
    raw = np.empty((len(RAW_ANGLE_KEYS), total), dtype=np.float64) if raw_angles else None
    from .engine import default_context
    check(_capi.load().cr_dssp_features(default_context()._h, ptr(backbone), ptr(is_pro), ptr(res_off), ptr(ca_off),
                                        ptr(atoms), ptr(classes), ptr(atom_off), num, ptr(points), len(points), ptr(out),
                                        ptr(codes), None if raw is None else ptr(raw)))
    secondary = codes.view("S1").astype("U1")          # byte 0 -> '' (no code); '0' where no residue maps
    result, raw_result = [], []
    for s in range(num):
        lo, hi = int(ca_off[s]), int(ca_off[s + 1])
        data = {}
        for row, key in enumerate(DSSP_KEYS):
            v = out[row, lo:hi].copy()
            data[key] = v.astype(np.int64) if key in INTEGER_KEYS else v
        data["secondary"] = secondary[lo:hi].copy()
        result.append(data)
        if raw_angles:
            raw_result.append({key: raw[row, lo:hi].copy() for row, key in enumerate(RAW_ANGLE_KEYS)})
    return (result, raw_result) if raw_angles else result


def _check_only_dssp(only_dssp):
    if not only_dssp:
        raise ValueError(_NOT_AVAILABLE)


def get_features(pdb_file, dssp_dir, only_dssp=True, force_overwrite=True, n_modes=50) -> dict:
    """feature_extraction.py:162-197 with only_dssp=True: the DSSP feature dict of one PDB file, one (L,) array per key
    over its C-alpha residues.  dssp_dir, force_overwrite and n_modes are accepted and unused (nothing is written and no
    external program runs).  No CPU fallback: without a device this raises CarettaHipError."""
    _check_only_dssp(only_dssp)
    return get_features_multiple([pdb_file], dssp_dir, 1, only_dssp, force_overwrite, n_modes)[0]


def get_features_multiple(pdb_files, dssp_dir, num_threads=20, only_dssp=True, force_overwrite=True,
                          n_modes=50) -> typing.List[dict]:
    """feature_extraction.py:128-159: get_features of every file, in order, computed in one batched device pass.
    num_threads is accepted and unused (the files are parsed on the host, then one device call does the rest)."""
    _check_only_dssp(only_dssp)
    structures = [structure_io.read_dssp_atoms(f) for f in pdb_files]
    return dssp_features_batch(structures)


def read_fasta(filename) -> typing.Tuple[typing.List[str], typing.List[str]]:
    names, rows = [], []
    for line in Path(filename).read_text().splitlines():
        line = line.strip()
        if not line:
            continue
        if line.startswith(">"):
            names.append(line[1:].strip())
            rows.append("")
        elif names:
            rows[-1] += line
        else:
            raise ValueError(f"{filename}: sequence before the first '>' header")
    return names, rows


def alignment_from_fasta(rows) -> typing.List[np.ndarray]:
    """'-' -> -1, every other character -> the running residue index."""
    out = []
    for row in rows:
        present = np.array([c != "-" for c in row], dtype=bool)
        idx = np.full(len(row), -1, dtype=np.int64)
        idx[present] = np.arange(int(present.sum()))
        out.append(idx)
    return out


def write_features(results_folder, verbose: bool = False) -> Path:
    """Add result_features.pkl (pickle of (names, aligned features)) to a results folder holding result.fasta and
    cleaned_pdb/<name>.pdb.  Every check runs before anything is written."""
    from . import helper
    from .multiple_alignment import get_aligned_features
    folder = Path(results_folder)
    if not folder.is_dir():
        raise ValueError(f"{folder}: not an existing results folder")
    fasta = folder / "result.fasta"
    if not fasta.is_file():
        raise ValueError(f"{fasta}: not found (write the alignment with --fasta / write_fasta=True)")
    cleaned = folder / "cleaned_pdb"
    names, rows = read_fasta(fasta)
    if not names:
        raise ValueError(f"{fasta}: no sequences")
    if len({len(r) for r in rows}) != 1:
        raise ValueError(f"{fasta}: the aligned rows differ in length")
    for name, row in zip(names, rows):
        pdb = cleaned / f"{name}.pdb"
        if not pdb.is_file():
            raise ValueError(f"{pdb}: not found")
        _, sequence = helper.read_calpha_pdb(pdb)
        if row.replace("-", "") != sequence:
            raise ValueError(f"{name}: the FASTA row does not match the C-alpha sequence of {pdb}")
    alignment = dict(zip(names, alignment_from_fasta(rows)))
    names, features = get_aligned_features(alignment, cleaned, folder / "tmp", num_threads=1)
    out = folder / "result_features.pkl"
    with open(out, "wb") as f:
        pickle.dump((names, features), f)
    if verbose:
        print(f"Aligned features: {out}")
    return out


def main(argv=None) -> int:
    import argparse
    parser = argparse.ArgumentParser(
        prog="python -m caretta_amd.feature_extraction",
        description="Add aligned DSSP features (result_features.pkl) to a results folder of align_from_structure_files. "
                    "The features follow Kabsch & Sander (1983) as DESIGN section 4.6 defines them; they are not mkdssp's.")
    parser.add_argument("results_folder", type=Path, help="folder with result.fasta and cleaned_pdb/")
    parser.add_argument("--verbose", "-v", action="store_true", help="print where the features were written")
    args = parser.parse_args(argv)
    try:
        write_features(args.results_folder, verbose=args.verbose)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
