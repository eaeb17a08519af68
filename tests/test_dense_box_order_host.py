"""The dense float4 grid's mapping from workgroup to box (csrc/kernels.hpp grid_eval_boxes), restated: the box list (z
fastest, then y, then x) is cut into chunks of 256; the workgroups of a chunk take its boxes, workgroup l of the chunk
(running on XCD l % 8) the (l // 8)-th box of that XCD's contiguous share.  Every box must be evaluated exactly once,
whatever the box count."""
import itertools

import pytest

CHUNK = 256     # kDenseChunk


def box_of_workgroup(i, n_boxes, chunk=CHUNK):
    first = i // chunk * chunk
    n = min(chunk, n_boxes - first)
    l = i - first
    k, q, r = l & 7, n >> 3, n & 7
    return first + k * q + min(k, r) + (l >> 3)


def is_permutation(n_boxes, chunk=CHUNK):
    return sorted(box_of_workgroup(i, n_boxes, chunk) for i in range(n_boxes)) == list(range(n_boxes))


def test_every_small_box_grid_is_covered_once():
    for shape in itertools.product(range(1, 10), repeat=3):
        n = shape[0] * shape[1] * shape[2]
        assert is_permutation(n), shape


def test_every_box_count_around_the_chunk_is_covered_once():
    for n in list(range(1, 2 * CHUNK + 18)) + [3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1, 3 * CHUNK + 7, 3 * CHUNK + 9]:
        assert is_permutation(n), n


def test_the_benchmark_grid_and_its_slabs_are_covered_once():
    from codecad_amd import dist
    assert is_permutation(32 * 32 * 32)
    for world in (2, 4, 8):
        for rank in range(world):
            begin, end = dist.x_slab(512, rank, world)
            planes = end - begin
            assert planes > 0
            assert is_permutation(((planes + 15) // 16) * 32 * 32), (rank, world)


def test_a_chunk_is_an_eighth_per_xcd_in_order():
    """workgroup i runs on XCD i % 8: inside a chunk each XCD walks a contiguous, ascending share, and the shares follow
    one another"""
    for n in (256, 9, 6, 77):
        shares = [[box_of_workgroup(i, n) for i in range(n) if i % 8 == k] for k in range(8)]
        flat = [b for s in shares for b in s]
        assert flat == list(range(n)), n


@pytest.mark.parametrize("chunk", [8, 64, 1024])
def test_any_multiple_of_eight_is_a_valid_chunk(chunk):
    for n in (1, 7, 8, 9, chunk - 1, chunk, chunk + 1, 2 * chunk + 5):
        assert is_permutation(n, chunk), (n, chunk)
