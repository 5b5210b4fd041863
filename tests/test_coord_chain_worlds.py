"""The worlds of coord_chain_worlds.py meet what the chain stage has to be tested on (CPU only: the oracle and the judge; the device
side is tests/test_gpu_chain_tables.py).  The thresholds are conditions on the test set.  These worlds are not the very ones the
conditions were first stated on: here the fourth sequence repeats 180 bp of the genome under label 0 (so that many k-mers carry
two coordinates of one label) before its new 150 bp, which is why far more (seed, label) pairs have several coordinates and more
tuples are cut than a fourth sequence of new sequence alone gives.  Next to each condition stands what THESE worlds give on the
oracle: ten worlds, 480 lists."""
import pytest

import coord_chain_worlds as ccw

N_WORLDS = 10


@pytest.fixture(scope="module")
def recipe_stats():
    stats = {}
    for seed in range(N_WORLDS):
        g, anno, reads = ccw.make_world(seed)
        lists = ccw.judge(g, ccw.make_config("recipe"), anno, reads, stats)
        assert len(lists) == 2 * len(reads)
    return stats


def test_the_recipe_chains(recipe_stats):
    s = recipe_stats
    assert s["lists"] == N_WORLDS * 48
    assert s["lists_with_a_back_pointer"] * 2 >= s["lists"], s           # these worlds: 377 of 480
    assert s["sub_k_seeds"] > 0, s                                        # these worlds: 2374
    assert s["multi_coordinate_pairs"] >= 20, s                           # these worlds: 6396


def test_sort_keys_are_unique(recipe_stats):
    """the oracle's std::sort is unstable: two anchors of a list must never share (label, coordinate, clipping, end)"""
    assert recipe_stats["duplicate_sort_keys"] == 0


def test_one_seed_per_locus_cuts_tuples():
    stats = {}
    for seed in range(N_WORLDS):
        g, anno, reads = ccw.make_world(seed)
        ccw.judge(g, ccw.make_config("one_per_locus"), anno, reads, stats)
    assert stats["tuples_cut"] > 0, stats                                 # these worlds: 6334
    assert stats["duplicate_sort_keys"] == 0


def test_the_filter_drops_a_label_and_empties_a_read():
    """min_exact_match = 0.7 on two reads.  The first lies across the joint of the fourth sequence (label 0): its first half is genome
    that the strain and the third sequence share, its second half is label 0's alone, so labels 1 and 2 cover about half of it
    and go while label 0 stays.  The second is random: the seeder itself leaves it without seeds."""
    import random
    g, anno, _, sequences = ccw.make_world(3, with_sequences=True)
    stats = {}
    lists = ccw.judge(g, ccw.make_config("exact_match"), anno, [sequences[3][130:230], ccw.rand_seq(random.Random(17), 100)], stats)
    assert stats["labels_dropped_with_one_kept"] >= 1, stats
    assert stats["lists_without_seeds"] >= 1, stats
    assert lists[0]["seeds"] and {a[0] for a in lists[0]["anchors"]} == {0}
    assert not lists[2]["seeds"] and not lists[3]["seeds"]


@pytest.mark.parametrize("world", ccw.kat_worlds(), ids=lambda w: w[0])
def test_kat_worlds_through_the_judge(world):
    name, g, anno, cfg, reads = world
    lists = ccw.judge(g, cfg, anno, reads)
    assert len(lists) == 2
    assert any(l["anchors"] for l in lists), name
