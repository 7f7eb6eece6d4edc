"""The site-block split of a partitioned alignment (dist.partition_site_blocks; the rule
rdamd_model_create_partitioned_block applies): every partition's OWN columns -- its ranges in
file order -- are chunked into G contiguous blocks the way dist.site_block chunks a whole
alignment (src/model.cpp:1899-1907: the first `mod` blocks take one extra column).  Checked
against hand-written ranges, uneven and shorter-than-G partitions included."""
import pytest

from root_digger_amd import dist


def test_equal_partitions_split_in_halves():
    parts = [[(1, 400)], [(401, 1000)]]
    assert dist.partition_site_blocks(parts, 0, 2) == [[(1, 200)], [(401, 700)]]
    assert dist.partition_site_blocks(parts, 1, 2) == [[(201, 400)], [(701, 1000)]]


def test_uneven_partitions_give_the_first_blocks_one_more_column():
    parts = [[(1, 7)], [(8, 17)], [(18, 1000)]]       # 7, 10 and 983 columns, four blocks
    want = {
        0: [[(1, 2)], [(8, 10)], [(18, 263)]],
        1: [[(3, 4)], [(11, 13)], [(264, 509)]],
        2: [[(5, 6)], [(14, 15)], [(510, 755)]],
        3: [[(7, 7)], [(16, 17)], [(756, 1000)]],
    }
    for b in range(4):
        assert dist.partition_site_blocks(parts, b, 4) == want[b]


def test_a_partition_of_several_ranges_is_split_over_its_own_columns():
    # columns 1-3 and 10-14 form one partition of 8 columns: blocks of 3, 3 and 2 of THEM
    parts = [[(1, 3), (10, 14)], [(4, 9)]]
    assert dist.partition_site_blocks(parts, 0, 3) == [[(1, 3)], [(4, 5)]]
    assert dist.partition_site_blocks(parts, 1, 3) == [[(10, 12)], [(6, 7)]]
    assert dist.partition_site_blocks(parts, 2, 3) == [[(13, 14)], [(8, 9)]]


def test_blocks_cover_every_partition_column_once():
    parts = [[(1, 5), (90, 101)], [(6, 89)], [(102, 103)]]
    for G in (1, 2):
        seen = [[] for _ in parts]
        for b in range(G):
            for p, ranges in enumerate(dist.partition_site_blocks(parts, b, G)):
                seen[p] += [c for lo, hi in ranges for c in range(lo, hi + 1)]
        assert seen == [[c for lo, hi in r for c in range(lo, hi + 1)] for r in parts]


def test_a_partition_shorter_than_the_site_blocks_is_refused_by_index():
    parts = [[(1, 100)], [(101, 103)]]                 # 3 columns, four blocks
    with pytest.raises(ValueError, match="partition 1 has 3 columns"):
        dist.partition_site_blocks(parts, 0, 4)
    assert dist.partition_site_blocks(parts, 2, 3)[1] == [(103, 103)]
    with pytest.raises(ValueError):
        dist.partition_site_blocks(parts, 4, 4)


def test_one_block_is_the_whole_partition():
    parts = [[(1, 300)], [(301, 1000)]]
    assert dist.partition_site_blocks(parts, 0, 1) == parts
