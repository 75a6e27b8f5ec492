"""Numpy model of the id matte and of the mask pulled from it, written from the text of include/pbrs_gpu.h ("id mattes") alone:
a table of `slots` (id, count) entries per pixel filled in sample-index order, first come, first kept; ranks by count, descending, the
lower id first among equal counts; the mask as a sum of the selected ranks' coverages in rank order."""
import numpy as np

MISS = 0xFFFFFFFF


def matte(insts_per_sample, key_of, slots):
    """insts_per_sample: (spp, P) u32, the instance of every sample's first hit in sample-index order, MISS where it hit nothing.
    key_of: None for the instance key, else a u32 array that maps an instance to its key (instances[i].material).
    -> ids (P, slots) u32, coverage (P, slots) f32, residual (P,) f32, and the integers behind them: counts (P, slots), overflow (P,)."""
    insts = np.asarray(insts_per_sample, dtype=np.uint32)
    spp, P = insts.shape
    ids = np.full((P, slots), MISS, dtype=np.uint32)
    counts = np.zeros((P, slots), dtype=np.uint32)
    overflow = np.zeros(P, dtype=np.uint32)
    for p in range(P):
        table = []  # [id, count], in the order the ids first came
        for s in range(spp):
            i = int(insts[s, p])
            if i == MISS:
                continue
            k = i if key_of is None else int(key_of[i])
            for entry in table:
                if entry[0] == k:
                    entry[1] += 1
                    break
            else:
                if len(table) < slots:
                    table.append([k, 1])
                else:
                    overflow[p] += 1
        table.sort(key=lambda e: (-e[1], e[0]))
        for r, (k, n) in enumerate(table):
            ids[p, r], counts[p, r] = k, n
    inv = np.float32(1.0) / np.float32(spp)
    coverage = (counts.astype(np.float32) * inv).astype(np.float32)
    residual = (overflow.astype(np.float32) * inv).astype(np.float32)
    return ids, coverage, residual, counts, overflow


def mask(ids, coverage, select):
    """ids, coverage: (..., slots); select: the selected ids, any order -> (...) f32: from +0, rank after rank, m = m + coverage[r] where
    ids[r] is selected."""
    ids = np.asarray(ids, dtype=np.uint32)
    coverage = np.asarray(coverage, dtype=np.float32)
    sel = np.unique(np.asarray(select, dtype=np.uint32))
    m = np.zeros(ids.shape[:-1], dtype=np.float32)
    for r in range(ids.shape[-1]):
        picked = np.isin(ids[..., r], sel)
        m = np.where(picked, (m + coverage[..., r]).astype(np.float32), m)
    return m
