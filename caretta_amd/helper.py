"""Numeric helpers of the reference's ``caretta/helper.py`` that sit on the pairwise path
(helper.py:13-42).  Integer work, done on the host inside libcaretta_hip."""
from __future__ import annotations

import ctypes as C

import numpy as np

from pathlib import Path

from . import _capi
from ._capi import check, i64, ptr

THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H",
                "ILE": "I", "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W",
                "TYR": "Y", "VAL": "V", "MSE": "M", "SEC": "U", "PYL": "O"}


def get_common_positions(aln_array_1, aln_array_2):
    """Positions where neither alignment row has a gap (-1)."""
    a1, a2 = i64(aln_array_1), i64(aln_array_2)
    if a1.shape != a2.shape:
        raise ValueError("alignment rows must have equal length")
    p1 = np.empty(max(len(a1), 1), np.int64)
    p2 = np.empty(max(len(a1), 1), np.int64)
    k = C.c_int64(0)
    check(_capi.load().cr_get_common_positions(ptr(a1), ptr(a2), len(a1), ptr(p1), ptr(p2), C.byref(k)))
    return p1[:k.value].copy(), p2[:k.value].copy()


def nb_mean_axis_0(array) -> np.ndarray:
    """Column means accumulated sequentially, as numba evaluates the reference's helper.nb_mean_axis_0
    (helper.py:46-53)."""
    x = np.ascontiguousarray(array, dtype=np.float64)
    out = np.empty(x.shape[1])
    check(_capi.load().cr_mean_axis0(ptr(x), x.shape[0], x.shape[1], ptr(out)))
    return out


def write_distance_matrix(names, distance_matrix, filename):
    """CLUSTAL-style text matrix: first line = count, then ``name v v v ...`` with 4 decimals
    (format of the reference's helper.write_distance_matrix, helper.py:183-202)."""
    matrix = np.asarray(distance_matrix, dtype=np.float64)
    if matrix.shape != (len(names), len(names)):
        raise ValueError("matrix shape does not match the number of names")
    with open(filename, "w") as handle:
        handle.write(f"{len(names)}\n")
        for name, row in zip(names, matrix):
            handle.write(name + " " + " ".join("%.4f" % value for value in row) + "\n")


def read_distance_matrix(filename):
    """Inverse of write_distance_matrix (helper.py:205-229): names (anything after a ``/`` dropped) and matrix."""
    with open(filename) as handle:
        count = int(handle.readline().strip())
        names, rows = [], []
        for line in handle:
            fields = line.split()
            if not fields:
                continue
            names.append(fields[0].strip().split("/")[0].strip())
            rows.append([float(v) for v in fields[1:count + 1]])
    if len(names) != count:
        raise ValueError(f"{filename}: header says {count} entries, found {len(names)}")
    return names, np.array(rows, dtype=np.float64).reshape(count, count)


def read_calpha_pdb(filename):
    """Minimal C-alpha reader standing in for parse_protein_files_and_clean (helper.py:161-180): ATOM/HETATM(MSE)
    records named CA of the FIRST chain of the FIRST model, first alternate location.
    Returns (coordinates float64 (L, 3), one-letter sequence)."""
    coords, seq = [], []
    chain = None
    seen = set()
    with open(filename) as handle:
        for line in handle:
            record = line[:6]
            if record.startswith("ENDMDL"):
                break
            if record not in ("ATOM  ", "HETATM") or line[12:16].strip() != "CA":
                continue
            resname = line[17:20].strip()
            if record == "HETATM" and resname != "MSE":
                continue
            if line[16] not in (" ", "A"):
                continue
            if chain is None:
                chain = line[21]
            elif line[21] != chain:
                break
            key = (line[22:27])
            if key in seen:
                continue
            seen.add(key)
            coords.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            seq.append(THREE_TO_ONE.get(resname, "X"))
    if not coords:
        raise ValueError(f"{filename}: no C-alpha atoms found")
    return np.array(coords, dtype=np.float64), "".join(seq)


def local_shape_descriptor(coordinates, width: int = 10):
    """Stand-in per-residue descriptor in [0, 1]^width for real structures when geometricus' learned
    embedding (the reference's tensor source, multiple_alignment.py:479-488) is not available:
    C-alpha distances to the residues at sequence offsets -k..+k (k = 2..), squashed with d / (d + 10 A).
    NOT the reference's tensors: results obtained with it are outside the parity contract."""
    x = np.asarray(coordinates, dtype=np.float64)
    length = x.shape[0]
    offsets = []
    k = 2
    while len(offsets) < width:
        offsets += [-k, k]
        k += 1
    out = np.zeros((length, width))
    for col, off in enumerate(offsets[:width]):
        idx = np.clip(np.arange(length) + off, 0, length - 1)
        dist = np.linalg.norm(x - x[idx], axis=1)
        out[:, col] = dist / (dist + 10.0)
    return out


def nb_std_axis_0(array) -> np.ndarray:
    """Column standard deviations (helper.py:57-64)."""
    return np.std(np.asarray(array, dtype=np.float64), axis=0)


def normalize(numbers) -> np.ndarray:
    """Min-max scaling to [0, 1] (helper.py:67-70)."""
    numbers = np.asarray(numbers, dtype=np.float64)
    lo, hi = np.min(numbers), np.max(numbers)
    return (numbers - lo) / (hi - lo)


# the stand-in tensor width of align_from_structure_files: 10 columns, alphabet of 2^10 shapemers
STANDIN_WIDTH = 10


def _pack_coordinates(coordinates_list):
    lists = [np.ascontiguousarray(x, dtype=np.float64) for x in coordinates_list]
    for x in lists:
        if x.ndim != 2 or x.shape[1] != 3 or x.shape[0] == 0:
            raise ValueError("each structure must be a non-empty (L, 3) array of coordinates")
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.shape[0] for x in lists], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(lists, axis=0)), offsets


def _split(flat, offsets):
    return [flat[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def structure_features(coordinates_list, width: int = STANDIN_WIDTH):
    """local_shape_descriptor(x, width) of every structure and its stand-in shapemer indices, in one device launch
    (cr_structure_features).  Returns (tensors: list of (L, width) float64, indices: list of (L,) int32).  The index of
    a residue is its row thresholded at 0.5 (a C-alpha distance of 10 A) read as a width-bit number, first column most
    significant: its position in itertools.product([0, 1], repeat=width), the key order of the reference
    (multiple_alignment.py:503).  NOT geometricus' shapemers: outside the parity contract."""
    from .engine import default_context
    coords, offsets = _pack_coordinates(coordinates_list)
    width = int(width)
    tensors = np.empty((coords.shape[0], max(width, 0)), dtype=np.float64)
    idx = np.empty(coords.shape[0], dtype=np.int32)
    check(_capi.load().cr_structure_features(default_context()._h, ptr(coords), ptr(offsets), len(offsets) - 1, width,
                                             ptr(tensors), ptr(idx)))
    return _split(tensors, offsets), _split(idx, offsets)


def structure_shapemer_distance_matrix(coordinates_list, width: int = STANDIN_WIDTH, return_features: bool = False):
    """The fast guide-tree matrix from coordinates: braycurtis(make_count_matrix(indices, 2^width), same) on the
    stand-in shapemers of structure_features, in one call (cr_structure_shapemer_distance_matrix; the indices never
    leave the device).  return_features: also (tensors, indices) as structure_features returns them."""
    from .engine import default_context
    coords, offsets = _pack_coordinates(coordinates_list)
    width, num = int(width), len(offsets) - 1
    out = np.empty((num, num), dtype=np.float64)
    tensors = np.empty((coords.shape[0], max(width, 0)), dtype=np.float64) if return_features else None
    idx = np.empty(coords.shape[0], dtype=np.int32) if return_features else None
    check(_capi.load().cr_structure_shapemer_distance_matrix(
        default_context()._h, ptr(coords), ptr(offsets), num, width, None if tensors is None else ptr(tensors),
        None if idx is None else ptr(idx), ptr(out)))
    if return_features:
        return out, _split(tensors, offsets), _split(idx, offsets)
    return out
