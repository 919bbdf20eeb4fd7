#!/usr/bin/env python3
"""Generate tests/golden/f11_braycurtis.npz by running the REFERENCE's own ``make_count_matrix`` and ``braycurtis``
(multiple_alignment.py:130-145, :390-396) and ``neighbor_joining`` on their result.

Run in the build container, where the reference tree exists (same stand-ins as generate_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/_gen/generate_shapemer_golden.py

The shapemer index lists are synthetic (geometricus is not installable): clades of related lists of about 2 x 300
indices, as geometricus' k-mer and radius shapemers give per residue.  Only inputs and outputs are written.

Case ``c<n>``: ``idx`` / ``off`` (CSR of the index lists), ``K``, ``counts`` = make_count_matrix(lists, K),
``D`` = braycurtis(counts, counts); ``tree`` / ``branches`` = neighbor_joining(D) where present.
Case ``r<n>`` (query against library): ``q_idx`` / ``q_off``, ``l_idx`` / ``l_off``, ``K``, ``q_counts``,
``l_counts``, ``D`` = braycurtis(q_counts, l_counts).
"""
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(HERE / "stubs"))
sys.path.insert(1, os.environ.get("CARETTA_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

from caretta import multiple_alignment, neighbor_joining  # noqa: E402

OUT = HERE.parent / "f11_braycurtis.npz"


def clade_lists(rng, num, k, length, clades, mutate=0.2):
    """num lists of about `length` indices in [0, k): members of a clade share a base list, each position is redrawn
    with probability `mutate`."""
    bases = [rng.integers(0, k, size=length) for _ in range(clades)]
    out = []
    for p in range(num):
        base = bases[p % clades]
        n = max(1, length + int(rng.integers(-length // 5, length // 5 + 1)))
        lst = rng.choice(base, size=n) if n != length else base.copy()
        redraw = rng.random(n) < mutate
        lst[redraw] = rng.integers(0, k, size=int(redraw.sum()))
        out.append(lst.astype(np.int64))
    return out


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    idx = np.concatenate(lists).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return idx, off


def main():
    rng = np.random.default_rng(20261015)
    out = {}
    cases = []
    # P = 2, K = 16: two short lists
    cases.append(([rng.integers(0, 16, size=40), rng.integers(0, 16, size=25)], 16))
    # P = 3, K = 16: a single-bin protein and empty bins
    cases.append(([np.full(30, 7), rng.integers(0, 8, size=50), rng.integers(4, 16, size=12)], 16))
    # P = 17, K = 1024: clades, a single-bin protein, two identical lists and a permutation of one (exact 0 off the
    # diagonal), most bins empty
    lists = clade_lists(rng, 17, 1024, 600, clades=3)
    lists[4] = np.full(90, 1023)
    lists[9] = lists[2].copy()
    lists[13] = rng.permutation(lists[5])
    cases.append((lists, 1024))
    # P = 64, K = 1024: six clades of ~2 x 300 indices
    cases.append((clade_lists(rng, 64, 1024, 600, clades=6), 1024))
    # P = 17, K = 16: dense bins, counts far above one per bin
    cases.append((clade_lists(rng, 17, 16, 300, clades=2, mutate=0.5), 16))
    # P = 64, K = 16
    cases.append((clade_lists(rng, 64, 16, 120, clades=4), 16))
    for c, (lists, k) in enumerate(cases):
        lists = [np.asarray(x, dtype=np.int64) for x in lists]
        counts = multiple_alignment.make_count_matrix(lists, k)
        d = multiple_alignment.braycurtis(counts, counts)
        idx, off = csr(lists)
        out.update({f"c{c}_idx": idx, f"c{c}_off": off, f"c{c}_K": np.int64(k), f"c{c}_counts": counts, f"c{c}_D": d})
        if len(lists) > 3:
            tree, branches = neighbor_joining.neighbor_joining(d)
            out[f"c{c}_tree"], out[f"c{c}_branches"] = tree, branches
    out["ncases"] = np.int64(len(cases))
    # query against library: 5 queries (one empty) x 23 library lists, K = 1024; and 3 x 2 at K = 16
    rect = [(clade_lists(rng, 5, 1024, 600, clades=2), clade_lists(rng, 23, 1024, 600, clades=4), 1024),
            (clade_lists(rng, 3, 16, 50, clades=1), clade_lists(rng, 2, 16, 20, clades=2), 16)]
    rect[0][0][3] = np.zeros(0, dtype=np.int64)
    rect[0][1][7] = rect[0][0][1].copy()
    for r, (q, lib, k) in enumerate(rect):
        qc = multiple_alignment.make_count_matrix(q, k)
        lc = multiple_alignment.make_count_matrix(lib, k)
        d = multiple_alignment.braycurtis(qc, lc)
        (qi, qo), (li, lo) = csr(q), csr(lib)
        out.update({f"r{r}_q_idx": qi, f"r{r}_q_off": qo, f"r{r}_l_idx": li, f"r{r}_l_off": lo, f"r{r}_K": np.int64(k),
                    f"r{r}_q_counts": qc, f"r{r}_l_counts": lc, f"r{r}_D": d})
    out["nrect"] = np.int64(len(rect))
    out["_numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print(f"  wrote {OUT.name}: {len(out)} arrays, {OUT.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
