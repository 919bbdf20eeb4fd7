"""Deterministic synthetic structure families.

The reference ships no benchmark inputs, so every configuration in
BASELINE.json is exercised on a *two-level clade family*: a random-walk
C-alpha trace, K clades derived from it by coordinate/tensor noise plus an
indel, and P/K members per clade derived the same way, each finally moved by a
random rigid motion.  Indels keep the length fixed (delete g residues, append g
fresh ones) so that every pair needs gaps.  All arrays are float64 C-contiguous,
as the reference's ``Protein`` expects (``multiple_alignment.py:312-319,486``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

CA_STEP = 3.8  # Angstrom between consecutive C-alpha atoms


@dataclass
class Structure:
    name: str
    tensors: np.ndarray  # (L, d) float64
    coordinates: np.ndarray  # (L, 3) float64
    sequence: str


def _walk(rng: np.random.Generator, length: int, start=None) -> np.ndarray:
    steps = rng.normal(size=(length, 3))
    steps /= np.linalg.norm(steps, axis=1, keepdims=True)
    steps *= CA_STEP
    trace = np.cumsum(steps, axis=0)
    if start is not None:
        trace = trace + start
    return trace


def _indel(rng, coords, tensors, gmax, append=True):
    g = int(rng.integers(0, gmax + 1)) if gmax > 0 else 0
    if g == 0:
        return coords, tensors
    length = coords.shape[0]
    start = int(rng.integers(0, length - g + 1))
    keep = np.r_[0:start, start + g:length]
    coords, tensors = coords[keep], tensors[keep]
    if append:
        tail = _walk(rng, g, start=coords[-1])
        coords = np.vstack([coords, tail])
        tensors = np.vstack([tensors, rng.uniform(size=(g, tensors.shape[1]))])
    return coords, tensors


def _random_rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_family(num: int, length: int, dim: int = 10, seed: int = 20240,
                ragged: bool = False, clades: int | None = None) -> List[Structure]:
    """P=``num`` structures of ``length`` residues with ``dim``-wide tensors."""
    rng = np.random.default_rng(seed)
    if clades is None:
        clades = 8 if num >= 32 else 4
    clades = max(1, min(clades, num))
    base = _walk(rng, length)
    t0 = rng.uniform(size=(length, dim))
    per = [num // clades + (1 if c < num % clades else 0) for c in range(clades)]
    out: List[Structure] = []
    for c in range(clades):
        xc = base + rng.normal(scale=2.0, size=base.shape)
        tc = t0 + rng.normal(scale=0.08, size=t0.shape)
        xc, tc = _indel(rng, xc, tc, length // 10)
        for _ in range(per[c]):
            x = xc + rng.normal(scale=1.0, size=xc.shape)
            t = tc + rng.normal(scale=0.03, size=tc.shape)
            x, t = _indel(rng, x, t, length // 20)
            if ragged:
                target = int(rng.integers(int(0.8 * length), length + 1))
                cut = x.shape[0] - target
                if cut > 0:
                    s = int(rng.integers(0, x.shape[0] - cut + 1))
                    keep = np.r_[0:s, s + cut:x.shape[0]]
                    x, t = x[keep], t[keep]
            rot = _random_rotation(rng)
            x = x @ rot + rng.uniform(-50.0, 50.0, size=3)
            idx = len(out)
            out.append(Structure(
                name=f"s{idx:04d}",
                tensors=np.ascontiguousarray(t, dtype=np.float64),
                coordinates=np.ascontiguousarray(x, dtype=np.float64),
                sequence="A" * x.shape[0],
            ))
    return out


def make_ragged_family(num: int, shortest: int, longest: int, dim: int = 10, seed: int = 20250, clades: int | None = None) -> List[Structure]:
    """A family whose members keep a random contiguous window of ``shortest`` .. ``longest`` residues of a ``longest``-residue
    family member each: ragged lengths as every real input has them (the reference's own example is 85 / 79 / 80 residues),
    still one family (related structures, alignments with gaps)."""
    fam = make_family(num, longest, dim=dim, seed=seed, clades=clades)
    rng = np.random.default_rng(seed + 7)
    for s in fam:
        keep = int(rng.integers(shortest, longest + 1))
        start = int(rng.integers(0, s.coordinates.shape[0] - keep + 1))
        s.coordinates = np.ascontiguousarray(s.coordinates[start:start + keep])
        s.tensors = np.ascontiguousarray(s.tensors[start:start + keep])
        s.sequence = s.sequence[start:start + keep]
    return fam


def make_mixed_family(num_short: int, short_len: int, num_long: int, long_len: int, dim: int = 10, seed: int = 20251) -> List[Structure]:
    """``num_short`` structures of ``short_len`` residues (windows of the long ones' family) followed by ``num_long`` members of
    ``long_len`` residues: a family of domains with a few full-length chains in it."""
    fam = make_family(num_short + num_long, long_len, dim=dim, seed=seed)
    rng = np.random.default_rng(seed + 11)
    for s in fam[:num_short]:
        start = int(rng.integers(0, long_len - short_len + 1))
        s.coordinates = np.ascontiguousarray(s.coordinates[start:start + short_len])
        s.tensors = np.ascontiguousarray(s.tensors[start:start + short_len])
        s.sequence = s.sequence[start:start + short_len]
    return fam


def pack(structures: List[Structure]):
    """Concatenate a family into the packed layout the C-ABI takes.

    Returns ``coords (sum L, 3)``, ``tensors (sum L, d)``, ``offsets int64 (P+1)``.
    """
    lens = [s.coordinates.shape[0] for s in structures]
    offsets = np.zeros(len(structures) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    coords = np.ascontiguousarray(np.vstack([s.coordinates for s in structures]), dtype=np.float64)
    tensors = np.ascontiguousarray(np.vstack([s.tensors for s in structures]), dtype=np.float64)
    return coords, tensors, offsets


def write_pdb_family(structures: List[Structure], folder) -> list:
    """Write a family as PDB files ``folder/<name>.pdb``: per residue N, CA, C and O (the N / C / O positions are
    fabricated around each C-alpha at bond-like distances; only the C-alpha atoms enter any fit).  Returns the paths."""
    from pathlib import Path
    folder = Path(folder)
    folder.mkdir(parents=True, exist_ok=True)
    around = {"N": (-1.20, 0.60, 0.30), "CA": (0.0, 0.0, 0.0), "C": (1.20, 0.55, -0.25), "O": (1.55, 1.70, -0.40)}
    paths = []
    for s in structures:
        lines, serial = [], 1
        for i, (x, aa) in enumerate(zip(s.coordinates, s.sequence)):
            res = {"A": "ALA", "G": "GLY"}.get(aa, "ALA")
            for atom, d in around.items():
                lines.append(f"ATOM  {serial:5d}  {atom:<3} {res} A{i + 1:4d}    {x[0] + d[0]:8.3f}{x[1] + d[1]:8.3f}"
                             f"{x[2] + d[2]:8.3f}  1.00  0.00           {atom[0]}")
                serial += 1
        path = folder / f"{s.name}.pdb"
        path.write_text("\n".join(lines) + "\nTER\nEND\n")
        paths.append(path)
    return paths


# ideal backbone geometry (Engh & Huber): bond lengths in A, bond angles in degrees
_BOND = {"N-CA": 1.458, "CA-C": 1.525, "C-N": 1.329, "C-O": 1.231}
_ANGLE = {"N-CA-C": 111.2, "CA-C-N": 116.2, "C-N-CA": 121.7, "CA-C-O": 120.5}


def _place(a, b, c, bond, angle, torsion):
    """NeRF: the atom d with |cd| = bond, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion (degrees)."""
    angle, torsion = np.radians(angle), np.radians(torsion)
    bc = c - b
    bc /= np.linalg.norm(bc)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d2 = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(torsion), bond * np.sin(angle) * np.sin(torsion)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * n


def ideal_backbone(phi, psi, omega=None) -> np.ndarray:
    """Backbone (L, 4, 3) -- N, CA, C, O per residue -- built by NeRF from per-residue phi / psi / omega in degrees (omega
    defaults to 180) with ideal bond lengths and angles.  phi[0] is unused; O lies in the peptide plane (dihedral
    N-CA-C-O = psi + 180)."""
    phi = np.asarray(phi, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)
    length = len(phi)
    omega = np.full(length, 180.0) if omega is None else np.asarray(omega, dtype=np.float64)
    out = np.zeros((length, 4, 3))
    out[0, 0] = (0.0, 0.0, 0.0)
    out[0, 1] = (_BOND["N-CA"], 0.0, 0.0)
    ang = np.radians(_ANGLE["N-CA-C"])
    out[0, 2] = out[0, 1] + _BOND["CA-C"] * np.array([-np.cos(ang), np.sin(ang), 0.0])
    for i in range(1, length):
        n_, ca_, c_ = out[i - 1, 0], out[i - 1, 1], out[i - 1, 2]
        out[i, 0] = _place(n_, ca_, c_, _BOND["C-N"], _ANGLE["CA-C-N"], psi[i - 1])
        out[i, 1] = _place(ca_, c_, out[i, 0], _BOND["N-CA"], _ANGLE["C-N-CA"], omega[i - 1])
        out[i, 2] = _place(c_, out[i, 0], out[i, 1], _BOND["CA-C"], _ANGLE["N-CA-C"], phi[i])
    for i in range(length):
        out[i, 3] = _place(out[i, 0], out[i, 1], out[i, 2], _BOND["C-O"], _ANGLE["CA-C-O"], psi[i] + 180.0)
    return out


def full_atom_structure(rng: np.random.Generator, length: int, side_atoms: float = 3.8):
    """A synthetic full-atom chain for timing the DSSP path: NeRF backbone from random helix / strand / coil phi-psi runs,
    a CB and pseudo side-chain atoms stepped outwards from it, about 4 + side_atoms heavy atoms per residue (7.8 by
    default, a protein's average).  Returns (backbone (L, 4, 3), atoms (A, 3), radius_class (A,), atom_offsets (L + 1,),
    is_pro (L,)): the arrays of structure_io.DsspAtoms with every residue complete."""
    states = np.array([[-57.8, -47.0], [-139.0, 135.0], [-70.0, 140.0]])
    phi, psi = np.empty(length), np.empty(length)
    i = 0
    while i < length:
        run = int(rng.integers(4, 16))
        s = states[int(rng.integers(0, 3))]
        phi[i:i + run] = s[0] + rng.normal(scale=6.0, size=min(run, length - i))
        psi[i:i + run] = s[1] + rng.normal(scale=6.0, size=min(run, length - i))
        i += run
    bb = ideal_backbone(phi, psi)
    is_pro = (rng.uniform(size=length) < 0.05).astype(np.int32)
    atoms, classes, counts = [], [], []
    for r in range(length):
        n_, ca, c_ = bb[r, 0], bb[r, 1], bb[r, 2]
        cb = _place(c_, n_, ca, 1.53, 110.5, -122.6)
        extra = int(rng.poisson(side_atoms - 1.0)) if side_atoms > 1.0 else 0
        side = [cb]
        for _ in range(extra):
            step = side[-1] - ca
            step /= np.linalg.norm(step)
            d = step + rng.normal(scale=0.35, size=3)
            side.append(side[-1] + 1.52 * d / np.linalg.norm(d))
        atoms += [bb[r, 0], bb[r, 1], bb[r, 2], bb[r, 3]] + side
        classes += [0, 1, 2, 3] + [4] * len(side)
        counts.append(4 + len(side))
    offsets = np.zeros(length + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    shift = rng.uniform(-50.0, 50.0, size=3)
    rot = _random_rotation(rng)
    bb = bb @ rot + shift
    atoms = np.asarray(atoms) @ rot + shift
    return (np.ascontiguousarray(bb), np.ascontiguousarray(atoms), np.array(classes, dtype=np.int32), offsets, is_pro)


def make_full_atom_family(num: int, shortest: int, longest: int, seed: int = 20260):
    """``num`` full_atom_structure chains of ``shortest`` .. ``longest`` residues as structure_io.DsspAtoms."""
    from .structure_io import DsspAtoms
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        length = int(rng.integers(shortest, longest + 1))
        bb, atoms, classes, offsets, is_pro = full_atom_structure(rng, length)
        out.append(DsspAtoms(length, np.ones(length, dtype=bool), bb, is_pro, offsets, atoms, classes))
    return out
