"""Structure-file input and output for ``align_from_structure_files`` without prody / geometricus: the semantics of the
reference's ``helper.parse_protein_files_and_clean`` (helper.py:161-180) and the PDB writing of its
``write_superposed_pdbs*`` (multiple_alignment.py:596-853), on plain PDB text.

Accepted inputs: a folder, a list of files or of ``(file, chain)`` tuples, or a text file listing one file per line
(optionally ``file, chain``).  Files are ``.pdb``, ``.ent`` or ``.pdb.gz``.  mmCIF is not read, and nothing is ever
downloaded: an input that is not an existing file or folder is a ``ValueError`` that names it.
"""
from __future__ import annotations

import gzip
import typing
from dataclasses import dataclass
from pathlib import Path

import numpy as np


STRUCTURE_SUFFIXES = (".pdb.gz", ".ent.gz", ".pdb", ".ent")
_UNSUPPORTED_SUFFIXES = (".cif", ".cif.gz", ".mmcif", ".bcif")


def structure_stem(path) -> str:
    """``x.pdb``, ``x.ent``, ``x.pdb.gz`` -> ``x``: the protein's name and the name of its cleaned file."""
    name = Path(path).name
    for suffix in STRUCTURE_SUFFIXES:
        if name.lower().endswith(suffix):
            return name[:-len(suffix)]
    return Path(path).stem


def _is_structure_file(path: Path) -> bool:
    return path.name.lower().endswith(STRUCTURE_SUFFIXES)


def _check_file(path: Path, what) -> Path:
    if not path.is_file():
        raise ValueError(f"{what!s}: not an existing structure file or folder (PDB IDs are not downloaded)")
    if path.name.lower().endswith(_UNSUPPORTED_SUFFIXES):
        raise ValueError(f"{path}: mmCIF input is not supported; convert it to PDB")
    if not _is_structure_file(path):
        raise ValueError(f"{path}: not a structure file (expected {', '.join(STRUCTURE_SUFFIXES)})")
    return path


def get_structure_files(input_value) -> typing.List[typing.Tuple[Path, typing.Optional[str]]]:
    """The structure files of an input and the chain asked for in each (None: the first chain)."""
    if isinstance(input_value, (list, tuple)):
        out = []
        for item in input_value:
            if isinstance(item, (list, tuple)):
                if len(item) != 2:
                    raise ValueError(f"{item!r}: expected (file, chain)")
                chain = None if item[1] is None else str(item[1]).strip() or None
                out.append((_check_file(Path(item[0]), item[0]), chain))
            else:
                out.append((_check_file(Path(item), item), None))
        return out
    path = Path(input_value)
    if path.is_dir():
        files = sorted(p for p in path.iterdir() if p.is_file() and _is_structure_file(p))
        cif = sorted(p for p in path.iterdir() if p.is_file() and p.name.lower().endswith(_UNSUPPORTED_SUFFIXES))
        if cif:
            raise ValueError(f"{cif[0]}: mmCIF input is not supported; convert it to PDB")
        return [(p, None) for p in files]
    if path.is_file() and _is_structure_file(path):
        return [(path, None)]
    if path.is_file():
        # a listing: one file per line, optionally "file, chain"; relative names are tried as given, then next to the list
        out = []
        for line in path.read_text().splitlines():
            line = line.strip()
            if not line:
                continue
            name, _, chain = (x.strip() for x in line.partition(","))
            f = Path(name)
            if not f.is_absolute() and not f.exists() and (path.parent / f).exists():
                f = path.parent / f
            out.append((_check_file(f, name), chain or None))
        return out
    raise ValueError(f"{input_value!s}: not an existing structure file or folder (PDB IDs are not downloaded)")


def _open_text(path: Path):
    if path.name.lower().endswith(".gz"):
        return gzip.open(path, "rt")
    return open(path)


def clean_pdb_lines(path, chain: typing.Optional[str] = None) -> typing.List[str]:
    """The records ``parse_protein_files_and_clean`` keeps: the first model, the chosen chain (default: the first one
    met), ATOM records and HETATM MSE, first alternate location (' ' or 'A') -- the rules of helper.read_calpha_pdb."""
    kept = []
    with _open_text(Path(path)) as handle:
        for line in handle:
            record = line[:6]
            if record.startswith("ENDMDL"):
                break
            if record not in ("ATOM  ", "HETATM"):
                continue
            if record == "HETATM" and line[17:20].strip() != "MSE":
                continue
            if line[16:17] not in (" ", "A"):
                continue
            if chain is None:
                chain = line[21:22]
            if line[21:22] != chain:
                continue
            kept.append(line.rstrip("\r\n"))
    if not kept:
        raise ValueError(f"{path}: no protein atoms" + (f" in chain {chain!r}" if chain else ""))
    return kept


def parse_protein_files_and_clean(input_value, output_folder, num_threads: int = 1) -> typing.List[Path]:
    """helper.py:161-180: every input structure reduced to its first model and chain, written to
    ``output_folder/<stem>.pdb``; returns those paths in input order.  Parsing runs on up to ``min(num_threads, 16)``
    threads (pure Python and file I/O: no library call is made)."""
    files = get_structure_files(input_value)
    stems = [structure_stem(f) for f, _ in files]
    seen = set()
    for f, s in zip(files, stems):
        if s in seen:
            raise ValueError(f"{f[0]}: a second structure named {s!r}")
        seen.add(s)
    output_folder = Path(output_folder)
    output_folder.mkdir(exist_ok=True)

    def one(job):
        (f, chain), stem = job
        out = output_folder / f"{stem}.pdb"
        out.write_text("\n".join(clean_pdb_lines(f, chain)) + "\nEND\n")
        return out

    workers = max(1, min(int(num_threads), 16))
    if workers == 1 or len(files) < 2:
        return [one(j) for j in zip(files, stems)]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(one, zip(files, stems)))


@dataclass
class PdbAtoms:
    """The atom records of a (cleaned) PDB file: every line as read, the coordinates of its ATOM / HETATM lines, and
    for every residue helper.read_calpha_pdb returns, the row of its C-alpha among those atoms."""
    lines: typing.List[str]
    atom_lines: np.ndarray      # (N,) int: line number of each atom row
    coords: np.ndarray          # (N, 3) float64
    ca_rows: np.ndarray         # (L,) int32


def read_pdb_atoms(filename) -> PdbAtoms:
    with _open_text(Path(filename)) as handle:
        lines = [line.rstrip("\r\n") for line in handle]
    atom_lines, coords, ca_rows = [], [], []
    chain, seen, other_chain = None, set(), False
    for n, line in enumerate(lines):
        record = line[:6]
        if record.startswith("ENDMDL"):
            break
        if record not in ("ATOM  ", "HETATM"):
            continue
        row = len(atom_lines)
        atom_lines.append(n)
        coords.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
        # the C-alpha selection of read_calpha_pdb, restated on the atom rows
        if (other_chain or line[12:16].strip() != "CA" or (record == "HETATM" and line[17:20].strip() != "MSE")
                or line[16] not in (" ", "A")):
            continue
        if chain is None:
            chain = line[21]
        elif line[21] != chain:          # (read_calpha_pdb stops at the first C-alpha of another chain)
            other_chain = True
            continue
        key = line[22:27]
        if key in seen:
            continue
        seen.add(key)
        ca_rows.append(row)
    if not ca_rows:
        raise ValueError(f"{filename}: no C-alpha atoms found")
    return PdbAtoms(lines, np.array(atom_lines, dtype=np.int64), np.array(coords, dtype=np.float64).reshape(-1, 3),
                    np.array(ca_rows, dtype=np.int32))


def _coordinate_field(value: float) -> str:
    text = "%8.3f" % value
    if len(text) != 8 or not np.isfinite(value):
        raise ValueError(f"coordinate {value!r} does not fit the 8 columns of a PDB coordinate field")
    return text


def write_pdb_atoms(filename, atoms: PdbAtoms, coords) -> None:
    """Every line of ``atoms`` copied, the coordinate columns 31-54 of its atom rows replaced by ``coords``
    (``%8.3f%8.3f%8.3f``).  A value that does not fit is a ValueError (nothing is written)."""
    coords = np.asarray(coords, dtype=np.float64)
    if coords.shape != atoms.coords.shape:
        raise ValueError("coordinates do not match the atom records")
    lines = list(atoms.lines)
    for row, n in enumerate(atoms.atom_lines):
        line = lines[n].ljust(54)
        lines[n] = line[:30] + "".join(_coordinate_field(v) for v in coords[row]) + line[54:]
    Path(filename).write_text("\n".join(lines) + "\n")


# radius classes of the DSSP accessibility (cr_dssp_features): N, CA, C, O by atom name, every other heavy atom
DSSP_RADIUS_CLASS = {"N": 0, "CA": 1, "C": 2, "O": 3}


@dataclass
class DsspAtoms:
    """What DSSP needs of a (cleaned) PDB file, over the residues helper.read_calpha_pdb returns (L of them): which are
    complete (N, CA, C and O present), the backbone and PRO flag of each complete residue, and the heavy atoms of the
    complete residues in file order with their radius class."""
    num_residues: int            # L: C-alpha residues
    complete: np.ndarray         # (L,) bool
    backbone: np.ndarray         # (R, 4, 3) float64: N, CA, C, O of the complete residues
    is_pro: np.ndarray           # (R,) int32
    atom_offsets: np.ndarray     # (R + 1,) int64: the heavy atoms of complete residue r
    atoms: np.ndarray            # (A, 3) float64
    radius_class: np.ndarray     # (A,) int32


def _element(line: str) -> str:
    element = line[76:78].strip() if len(line) >= 78 else ""
    if element:
        return element.upper()
    name = line[12:16].strip().lstrip("0123456789")
    return name[:1].upper()


def read_dssp_atoms(filename) -> DsspAtoms:
    """Residues as read_pdb_atoms selects them (first model, first chain, first altloc, HETATM MSE counted), every
    ATOM / HETATM MSE record of those residues with altloc ' ' or 'A' assigned to its residue; hydrogens (element H or D)
    are dropped, OXT is kept.  The first N / CA / C / O of a residue make its backbone."""
    pdb = read_pdb_atoms(filename)
    lines = pdb.lines
    first = lines[pdb.atom_lines[pdb.ca_rows[0]]]
    chain = first[21]
    residue_of = {}
    for i, row in enumerate(pdb.ca_rows):
        residue_of[lines[pdb.atom_lines[row]][22:27]] = i
    num = len(pdb.ca_rows)
    heavy = [[] for _ in range(num)]        # (row, name) per residue, file order
    backbone = [dict() for _ in range(num)]
    resname = [lines[pdb.atom_lines[row]][17:20].strip() for row in pdb.ca_rows]
    for row, n in enumerate(pdb.atom_lines):
        line = lines[n]
        if line[21] != chain or line[16] not in (" ", "A"):
            continue
        if line[:6] == "HETATM" and line[17:20].strip() != "MSE":
            continue
        i = residue_of.get(line[22:27])
        if i is None or _element(line) in ("H", "D"):
            continue
        name = line[12:16].strip()
        heavy[i].append((row, name))
        if name in DSSP_RADIUS_CLASS and name not in backbone[i]:
            backbone[i][name] = row
    complete = np.array([len(b) == 4 for b in backbone], dtype=bool)
    bb_rows, pro, atom_rows, classes, counts = [], [], [], [], []
    for i in np.flatnonzero(complete):
        bb_rows.append([backbone[i][a] for a in ("N", "CA", "C", "O")])
        pro.append(1 if resname[i] == "PRO" else 0)
        counts.append(len(heavy[i]))
        for row, name in heavy[i]:
            atom_rows.append(row)
            classes.append(DSSP_RADIUS_CLASS.get(name, 4))
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    bb = pdb.coords[np.array(bb_rows, dtype=np.int64).reshape(-1)].reshape(-1, 4, 3)
    return DsspAtoms(num, complete, np.ascontiguousarray(bb), np.array(pro, dtype=np.int32), offsets,
                     np.ascontiguousarray(pdb.coords[np.array(atom_rows, dtype=np.int64)].reshape(-1, 3)),
                     np.array(classes, dtype=np.int32))
