"""Several ranks sharing ONE GPU through gloo (host-staged collectives): the real multi-rank pipelines -- the HIP kernels,
the level launches' world and rank, hu_slice_rows -- of dist.mass_properties and dist.subdivision, compared with the single-GPU drivers.

Worlds of 2 and 3 ranks are spawned in turn, each under three replication settings (CODECAD_AMD_REPLICATE_SAMPLES = 0:
every level exchanged; the default; a huge value: every non-leaf level replicated).  Every rank reports through a queue;
the parent stops at the first rank that fails, exits with a signal or runs out of time, kills the others and starts
nothing more.  At most 3 ranks (and the test process) have the GPU open at once."""
import os
import queue as queue_module
import socket
import sys
import time
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

# (label, CODECAD_AMD_REPLICATE_SAMPLES: None = the default)
SETTINGS = (("exchanged", "0"), ("default", None), ("replicated", str(1 << 40)))
WORLDS = (2, 3)
GROUP_SECONDS = 300     # one world under one setting: start-up, two in-process builds, every case


def _shapes():
    import codecad_amd as cc
    s = cc.shapes
    empty = s.box(40) - s.sphere(100)      # the sphere holds the box: nothing is left, every list below the top goes empty
    return {
        "sphere_plus_box": cc.examples.sphere_plus_box,
        "sponge3": lambda: cc.examples.sponge(3),
        "planetary": cc.examples.planetary,                        # a pruned tape: the box masks are used
        "ring2d": lambda: s.circle(60) - s.rectangle(20, 20),
        "empty": lambda: empty,
        "speck": lambda: empty + s.sphere(2).translated(15, 15, 15),   # a small part far inside a large bounding box
    }


# (name, shape, resolution, grid, CODECAD_AMD_SPECIALIZE); all mass cases have three levels, replicate 2 by default;
# sphere_plus_box at 0.5, grid 8 has inside cells at level 0 (5^3 cells of 32: at res 1, 3^3 cells of 64, it has none)
MASS_CASES = (("spb_interp", "sphere_plus_box", 0.5, 8, "0"), ("spb_spec", "sphere_plus_box", 0.5, 8, "1"),
              ("sponge3", "sponge3", 1 / 243, 9, "0"), ("planetary", "planetary", 1.0, 8, "0"))
SUB_CASES = MASS_CASES + (("ring2d", "ring2d", 0.25, 8, "0"), ("one_block", "sphere_plus_box", 20.0, 16, "0"),
                          ("empty", "empty", 0.5, 8, "0"), ("speck", "speck", 0.5, 8, "0"))


def _free_port():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _sorted_rows(a):
    a = np.asarray(a)[:, :3]
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def _rank_cases(rank, label):
    """Everything one rank runs (all ranks the same calls, in the same order: the collectives pair up)."""
    import torch
    import codecad_amd as cc
    from codecad_amd import dist, nodes
    from codecad_amd.mass_properties import finish, _KEYS

    makers, shapes = _shapes(), {}

    def shape_of(name, policy):
        # one shape object (and so one uploaded tape) per shape and evaluator; the policy is read at upload
        if (name, policy) not in shapes:
            os.environ["CODECAD_AMD_SPECIALIZE"] = policy
            shapes[name, policy] = makers[name]()
            nodes.make_program_buffer(shapes[name, policy])
        return shapes[name, policy]

    device = torch.device("cuda", dist.local_device())
    stream = torch.cuda.current_stream(device).cuda_stream
    out = {"mass": {}, "sub": {}, "mass_single": {}, "sub_single": {}}
    for case, name, res, grid, policy in MASS_CASES:
        shape = shape_of(name, policy)
        box = shape.bounding_box()
        levels, capacities = dist.mass_hierarchy(box, res, grid)
        pipe = dist.MassPipeline(nodes.make_program_buffer(shape), levels, (box.a.x, box.a.y, box.a.z), capacities, device, stream)
        pipe.enqueue()
        pipe.finish()
        level0 = float(dist.allreduce_sum(pipe.pieces[0].sum(dim=0))[0])   # level 0's inside volume, summed over the ranks
        got = dist.mass_properties(shape, res, grid_size=grid)
        tape = nodes.make_program_buffer(shape)
        out["mass"][case] = dict(volume=got.volume, centroid=list(got.centroid), inertia=np.asarray(got.inertia_tensor).tolist(),
                                 replicate=pipe.pipe.replicate, levels=len(levels), specialized=bool(tape.specialized), level0=level0,
                                 extent=max(box.size()))
        del pipe
        if rank == 0:
            want = cc.mass_properties(shape, res, grid_size=grid)
            out["mass_single"][case] = dict(volume=want.volume, centroid=list(want.centroid), inertia=np.asarray(want.inertia_tensor).tolist())
    if label == "default":
        # a first try that overflows (lists of one row) and replicates both non-leaf levels; its repeat, with grown lists,
        # replicates one: nothing of the first try may reach the result
        shape = shape_of("sphere_plus_box", "0")
        box = shape.bounding_box()
        levels, _ = dist.mass_hierarchy(box, 0.5, 8)
        limit, dist.REPLICATE_MAX_SAMPLES = dist.REPLICATE_MAX_SAMPLES, 512 * 8
        tries = []
        try:
            partial = dist.mass_partial(nodes.make_program_buffer(shape), levels, (box.a.x, box.a.y, box.a.z), [1] * (len(levels) - 1),
                                        device, stream, tries)
        finally:
            dist.REPLICATE_MAX_SAMPLES = limit
        got = finish(dict(zip(_KEYS, dist.allreduce_sum(partial).tolist())))
        out["retry"] = dict(volume=got.volume, centroid=list(got.centroid), inertia=np.asarray(got.inertia_tensor).tolist(),
                            tries=[k for k, _ in tries], extent=max(box.size()))
    for case, name, res, grid, policy in SUB_CASES:
        shape = shape_of(name, policy)
        leaves, info = dist.subdivision(shape, res, grid_size=grid)
        box = shape.bounding_box().expanded_additive(res / 2)
        n_levels = len(cc.subdivision.calculate_block_sizes(box.flattened() if shape.dimension() == 2 else box, shape.dimension(), res, grid, True))
        out["sub"][case] = dict(leaves=_sorted_rows(leaves.cpu().numpy()), share=info["share"].cpu().numpy()[:, :3].copy(),
                                counts=list(info["level_counts"]), replicate=info["replicate"], levels=n_levels)
        if rank == 0:
            single = cc.subdivision.subdivision_device(shape, res, grid_size=grid)
            out["sub_single"][case] = dict(leaves=single.int_corners(), counts=list(single.level_counts))
    return out


def _rank(rank, world, port, samples, label, log, queue):
    fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 1)
    os.dup2(fd, 2)
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                          CODECAD_AMD_DIST_BACKEND="gloo", CODECAD_AMD_FORCE_COLLECTIVES="0")
        os.environ.pop("CODECAD_AMD_REPLICATE_SAMPLES", None)
        if samples is not None:
            os.environ["CODECAD_AMD_REPLICATE_SAMPLES"] = samples     # before codecad_amd.dist is imported: read at import
        sys.path.insert(0, ROOT)
        from codecad_amd import dist
        assert dist.REPLICATE_MAX_SAMPLES == (int(samples) if samples is not None else 4 << 20)
        assert dist.init() == (rank, world)
        result = _rank_cases(rank, label)
        queue.put((rank, "ok", result))
        dist.barrier()
        import torch.distributed
        torch.distributed.destroy_process_group()
    except BaseException:
        queue.put((rank, "error", traceback.format_exc()))
        raise


def _run_group(world, label, samples, logdir):
    """One world under one setting -> {rank: result}; fails (after killing every rank) at the first rank that fails."""
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    port = _free_port()
    logs = [os.path.join(logdir, "world%d_%s_rank%d.log" % (world, label, r)) for r in range(world)]
    procs = [ctx.Process(target=_rank, args=(r, world, port, samples, label, logs[r], queue)) for r in range(world)]
    results, failure = {}, None
    deadline = time.monotonic() + GROUP_SECONDS
    try:
        for p in procs:
            p.start()
        while failure is None and (len(results) < world or any(p.exitcode is None for p in procs)):
            try:
                r, status, payload = queue.get(timeout=0.5)
                if status == "ok":
                    results[r] = payload
                else:
                    failure = (r, "raised:\n" + payload)
            except queue_module.Empty:
                pass
            for r, p in enumerate(procs):
                if failure is None and p.exitcode not in (None, 0):
                    failure = (r, "exit status %d" % p.exitcode)
            if failure is None and time.monotonic() > deadline:
                failure = (None, "no result within %d s" % GROUP_SECONDS)
        if failure is None and len(results) < world:
            failure = (None, "ranks exited without a result: %s" % sorted(set(range(world)) - set(results)))
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
        for p in procs:
            p.join(timeout=30)
    if failure is not None:
        r, why = failure
        tails = []
        for k, path in enumerate(logs):
            if r is None or k == r:
                try:
                    with open(path, errors="replace") as f:
                        tails.append("--- rank %d ---\n%s" % (k, f.read()[-4000:]))
                except OSError:
                    pass
        pytest.fail("world %d, %s: rank %s: %s\n%s" % (world, label, r, why, "\n".join(tails)), pytrace=False)
    return results


def _check_mass(got, want, extent, where):
    assert abs(got["volume"] - want["volume"]) <= 1e-13 * abs(want["volume"]), (where, got["volume"], want["volume"])
    assert np.allclose(got["centroid"], want["centroid"], rtol=0, atol=1e-14 * extent), (where, got["centroid"], want["centroid"])
    scale = np.abs(np.asarray(want["inertia"])).max()
    assert np.allclose(got["inertia"], want["inertia"], rtol=1e-11, atol=1e-11 * scale), (where, got["inertia"], want["inertia"])


def _check_group(world, label, results):
    from codecad_amd import dist
    single = results[0]
    for case, name, res, grid, policy in MASS_CASES:
        where = (world, label, case)
        want = single["mass_single"][case]
        first = results[0]["mass"][case]
        assert first["levels"] == 3, where
        intended = {"exchanged": 0, "default": 2, "replicated": first["levels"] - 1}[label]
        for rank in range(world):
            got = results[rank]["mass"][case]
            assert got["replicate"] == intended, (where, rank, got["replicate"])
            assert got["specialized"] == (policy == "1"), (where, rank)
            if name == "sphere_plus_box":       # what makes the case mean something: solid material at level 0
                assert got["level0"] > 0, (where, rank)
            # every rank returns identical numbers
            assert (got["volume"], got["centroid"], got["inertia"]) == (first["volume"], first["centroid"], first["inertia"]), (where, rank)
        _check_mass(first, want, first["extent"], where)
    if label == "default":
        want = single["mass_single"]["spb_interp"]
        for rank in range(world):
            retry = results[rank]["retry"]
            assert len(retry["tries"]) >= 2 and retry["tries"][0] == 2 and retry["tries"][-1] == 1, (world, rank, retry["tries"])
            _check_mass(retry, want, retry["extent"], (world, label, "retry", rank))
    for case, name, res, grid, policy in SUB_CASES:
        where = (world, label, case)
        want = single["sub_single"][case]
        n = want["leaves"].shape[0]
        shares = []
        for rank in range(world):
            got = results[rank]["sub"][case]
            assert np.array_equal(got["leaves"], want["leaves"]), (where, rank, got["leaves"].shape, want["leaves"].shape)
            assert got["counts"] == want["counts"], (where, rank, got["counts"], want["counts"])
            pipeline_levels = got["levels"] - 1
            if label == "exchanged":
                assert got["replicate"] == 0, (where, rank)
            elif label == "replicated":
                assert got["replicate"] == pipeline_levels, (where, rank, got["replicate"])
            share = got["share"].shape[0]
            if pipeline_levels == 0:             # one leaf block: rank 0's
                assert share == (1 if rank == 0 else 0), (where, rank, share)
            elif got["replicate"] < pipeline_levels:     # the leaves came through hu_slice_rows: balanced slices
                b, e = dist.balanced_slice(n, rank, world)
                assert share == e - b, (where, rank, share, e - b)
            else:                                # owned: as even as a hash is (the gloo test's bound, plus 4 sigma)
                assert abs(share - n / world) <= 0.2 * n / world + 2 + 4 * (n / world) ** 0.5, (where, rank, share, n)
            shares.append(got["share"])
        # the shares tile the leaves, no overlap
        assert np.array_equal(_sorted_rows(np.concatenate(shares)), want["leaves"]), where
    assert single["sub_single"]["empty"]["leaves"].shape[0] == 0 and 0 in single["sub_single"]["empty"]["counts"]
    assert single["sub_single"]["speck"]["leaves"].shape[0] > 0
    assert single["sub_single"]["one_block"]["counts"] == []


def test_ranks_sharing_one_gpu_equal_one_gpu(tmp_path):
    """dist.mass_properties and dist.subdivision on 2 and 3 ranks equal the single-GPU drivers: the solid sphere_plus_box
    at grid 8 (two replicated levels, solid at level 0) under both evaluators, sponge(3), planetary's pruned tape; for
    subdivision also a 2D shape, a one-block hierarchy and lists that go empty; and a mass integration whose first try
    overflows with a different `replicate` from its repeat."""
    sys.path.insert(0, ROOT)
    for world in WORLDS:
        for label, samples in SETTINGS:
            results = _run_group(world, label, samples, str(tmp_path))
            _check_group(world, label, results)
