"""Folded chains (csrc/specialise.hpp fold_chains) on the device: the distance walks over boxes read one column per plane
where they read one per (plane, level), and every float stays the oracle's.  Shapes built to make the terms of a fold TIE:
unions of equal rectangles and crosses at several dyadic scales, sampled on dyadic lattices (exact zeros, equal distances
of different levels), in plain and mirrored frames, behind repetitions (nothing to prune, so the fold fires) and without
(box pruning decides, so it does not).  Both layouts of the dense kernel, leaf blocks, and the classification kernels over
boxes."""
import random

import numpy as np
import pytest

from test_gpu_bricks import check_classify, run

pytestmark = pytest.mark.gpu


def _shapes():
    import codecad_amd as cc
    s = cc.shapes
    bar = s.box(0.25, 0.25, float("inf"))
    cross = bar + bar.rotated_x(90) + bar.rotated_y(90)
    square = s.rectangle(0.25, 0.25).extruded(float("inf"))
    rep = s.unsafe.Repetition
    return {
        "equal_crosses": s.box() - rep(cross.scaled(0.5) + cross.scaled(0.5) + cross.scaled(0.25), (1.0, 1.0, 1.0)),
        "crosses_at_scales": s.box() - s.union(rep(cross.scaled(f), (f, f, f)) for f in (1.0, 0.5, 0.25, 0.125)),
        "mirrored_levels": s.box() - rep(cross.scaled(0.5) + cross.scaled(0.25).mirrored_x() + cross.rotated_z(90).scaled(0.125), (1.0, 1.0, 1.0)),
        "equal_rectangles": s.box(2, 2, 1) - rep(square + square.scaled(0.5) + square.translated(0.125, 0, 0).scaled(0.5), (0.5, 0.5, 1.0)),
        "pruned_crosses": s.box() - (cross.scaled(0.5) + cross.scaled(0.25)),
        "sponge3": cc.examples.sponge(3),
    }


@pytest.mark.parametrize("name", sorted(_shapes()))
def test_folded_distance_walks_match_the_oracle(hip, name, monkeypatch):
    from codecad_amd import hip_util, nodes
    tape = nodes.make_program(_shapes()[name])
    grids = [(np.array([-0.5, -0.5, -0.5]), np.float32(1 / 32), (32, 32, 32)),        # dyadic: samples on the bars' faces
             (np.array([-0.5, -0.5, -0.5]), np.float32(1 / 16), (16, 16, 24)),
             (np.array([-0.53, -0.49, -0.51]), np.float32(0.037), (20, 12, 40))]      # boxes cut by the grid's edge
    blocks = [([(0, 0, 0), (16, 0, 0), (-16, 16, -16), (5, -7, 3)], 1 / 32, (-0.5, -0.5, -0.5)),
              ([(0, 0, 0), (3, 9, -4)], 0.0625, (-0.5, -0.5, -0.5), (16, 8, 24))]
    run(hip, tape, grids, blocks)
    handle = hip_util.Tape(tape)
    handle.specialize()
    monkeypatch.setenv("HU_CLASSIFY_BOX_MIN", "1")     # (by default only launches of thousands of boxes go over boxes)
    rng = random.Random(hash(name) & 0xffff)
    for corner, step, dims in grids + [(np.array([-0.5, -0.5, -0.5]) + rng.uniform(-0.02, 0.02), np.float32(1 / 21), (21, 19, 13))]:
        check_classify(hip, handle, tape, corner, step, dims)
    handle.release()
