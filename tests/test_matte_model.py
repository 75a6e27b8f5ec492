"""The numpy model of the id matte (tests/matte_model.py, from the text of include/pbrs_gpu.h) against a brute-force count per pixel
on the oracle's first hits, without a GPU."""
import collections

import numpy as np
import pytest

import matte_model
from common import GOLDEN_NAMES
from matte_common import MISS, first_hits


@pytest.mark.parametrize("name", GOLDEN_NAMES)
@pytest.mark.parametrize("strata", [(2, 2), (4, 4)])
@pytest.mark.parametrize("slots", [1, 2, 6])
@pytest.mark.parametrize("key", ["instance", "material"])
def test_model_against_a_counter_per_pixel(name, strata, slots, key):
    insts, _, mat_of = first_hits(name, *strata)
    spp, P = insts.shape
    key_of = mat_of if key == "material" else None
    ids, coverage, residual, counts, overflow = matte_model.matte(insts, key_of, slots)
    inv = np.float32(1.0) / np.float32(spp)
    n_hit = (insts != MISS).sum(axis=0)
    exact = 0
    for p in range(P):
        hit = insts[:, p][insts[:, p] != MISS]
        brute = collections.Counter(int(i) if key_of is None else int(key_of[i]) for i in hit)
        used = counts[p] > 0
        got = {int(i): int(n) for i, n in zip(ids[p][used], counts[p][used])}
        assert len(got) == used.sum()  # no id twice
        if len(brute) <= slots:
            assert got == dict(brute) and overflow[p] == 0, p
            exact += 1
        else:
            assert used.all() and all(brute[i] == n for i, n in got.items()), p  # what is kept is counted in full
        assert counts[p].sum() + overflow[p] == n_hit[p]
        # ranks: used first, by count descending, the lower id first among equals; unused: MISS, +0
        order = [(-int(n), int(i)) for i, n in zip(ids[p][used], counts[p][used])]
        assert order == sorted(order) and used[:int(used.sum())].all()
        assert (ids[p][~used] == MISS).all() and (coverage[p][~used].view(np.uint32) == 0).all()
    assert exact > 0
    # power-of-two spp: every coverage is a multiple of 1 / spp and the sums are exact, so the mask of all ids plus the residual is
    # the coverage AOV's expression, bit for bit
    everything = np.unique(ids)
    m = matte_model.mask(ids, coverage, everything)
    total = (m + residual).astype(np.float32)
    assert (total.view(np.uint32) == (n_hit.astype(np.float32) * inv).astype(np.float32).view(np.uint32)).all()


def test_the_inputs_reach_every_branch():
    """What the GPU test leans on (tests/test_gpu_matte.py): pixels with several ids, overflow at 2 slots, none at 6."""
    insts, _, _ = first_hits("c5_many_lights", 4, 4)
    distinct = np.array([len(set(insts[:, p][insts[:, p] != MISS].tolist())) for p in range(insts.shape[1])])
    assert (distinct > 2).sum() > 0 and (distinct > 4).sum() > 0 and distinct.max() <= 6
    assert matte_model.matte(insts, None, 2)[4].any() and not matte_model.matte(insts, None, 6)[4].any()
    insts, _, _ = first_hits("c2_cornell_diffuse", 4, 4)
    assert (np.array([len(set(insts[:, p][insts[:, p] != MISS].tolist())) for p in range(insts.shape[1])]) > 1).sum() > 50


def test_mask_rules():
    ids = np.array([[[3, 7, MISS]], [[7, 1, 3]]], dtype=np.uint32)
    cov = np.array([[[0.5, 0.25, 0.0]], [[0.5, 0.25, 0.125]]], dtype=np.float32)
    assert matte_model.mask(ids, cov, []).tolist() == [[0.0], [0.0]]
    assert matte_model.mask(ids, cov, [7]).tolist() == [[0.25], [0.5]]
    assert matte_model.mask(ids, cov, [3, 7, 7]).tolist() == [[0.75], [0.625]]
    assert matte_model.mask(ids, cov, [99, MISS]).tolist() == [[0.0], [0.0]]


def test_the_kernels_sorting_network_sorts_every_table_size():
    """k_matte_finalize ranks with a fixed compare-exchange network whose comparators beyond `slots` are left out (device/matte.h):
    by the 0-1 principle it sorts, descending, for every slots = 1 .. 8."""
    import itertools
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrs_amd", "csrc", "device", "matte.h")).read()
    body = text[text.index("PD void matte_sort"):]
    net = [(int(i), int(j)) for i, j in re.findall(r"matte_cx<SLOTS, (\d), (\d)>\(e\)", body[:body.index("\n}\n")])]
    assert len(net) == 19 and all(i < j < 8 for i, j in net)
    for n in range(1, 9):
        for word in itertools.product((0, 1), repeat=n):
            e = list(word)
            for i, j in net:
                if i < n and j < n and e[j] > e[i]:
                    e[i], e[j] = e[j], e[i]
            assert e == sorted(word, reverse=True), (n, word)
