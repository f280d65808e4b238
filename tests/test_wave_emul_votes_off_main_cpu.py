"""CPU: ExpRunner.votes_off_main on the emulated wavefront (tests/wave_emul/: the product's kernel sources and the host layer's own
text compiled for x86-64).  The host's new ordering -- early stop and survivor scan on the main stream, ONE event, votes and stat
update on the tail stream, octree_ready_ev_ recorded there, the main stream's wait at the end of the step -- is its own code here:
the streams it asks for, the events it records and waits on.  What a stand-in without asynchrony can check is checked: training steps
with the knob at 1 give the bytes of the steps with the fused launches, across a compaction and a subdivision (maintenance
iterations keep the fused launches and must find the tail stream's updates behind them), with leaves dying under batches sampled two
steps ahead; and no stream was made to wait on an event nobody had recorded.  (Test infrastructure only; see
tests/test_wave_emul_cpu.py for the fixtures.  The file's name sorts it behind that module on purpose: the emulated host module is
loaded with its kernel library's symbols global, and the tests there that load a second build of the library -- reference numerics,
the deliberately broken kernels -- must have run before any host test does.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_wave_emul_cpu import emul_host, emul_lib, hip, rt  # noqa: F401  (fixtures)

R, NE, ITERS = 64, 64, 9


def run_steps(rt, st, knob, depth):
    import test_gpu_e2e as e2e
    overrides = ["field.log2_table_size=12", "train.learning_rate=0.0", "pts_sampler.sub_div_milestones=[7]", "pts_sampler.compact_freq=5"]
    rng0 = np.random.default_rng(31)
    batches = []
    for _ in range(ITERS + 2):
        ro, rd, bounds, cam = e2e.fox_batch(st, rng0, R)
        batches.append([torch.from_numpy(np.ascontiguousarray(a)) for a in (ro, rd, bounds, rng0.random((R, 3), dtype=np.float32), cam)])
    runner, cfg, _ = rt.make_runner(st, "wanjinyou", overrides, seed=5, table_init=0.3)
    states = [t.clone() for t in runner.states()]
    states[8][-16 * 64:-15 * 64] *= 16.0  # (a density that kills leaves: the scenario of tests/wave_emul/stream_races.py)
    runner.load_states(states)
    runner.n_edge_pts = NE
    runner.speculative_sampling, runner.speculation_depth, runner.march_blocks = True, depth, 96
    runner.votes_off_main = knob
    torch.manual_seed(11)
    losses = []
    for it in range(ITERS):
        for t in runner.occupancy_buffers()[:2]:
            t.fill_(0)
        b, nb, nb2 = batches[it], batches[it + 1], batches[it + 2]
        if depth >= 2:
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2], nb2[0], nb2[1])
        else:
            s = runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])
        losses.append(float(s["loss"]))
    runner.flush()
    out = dict(states=[t.detach().contiguous().numpy().tobytes() for t in runner.states()], nodes=runner.tree_nodes().numpy().tobytes(),
               occ=[t.numpy().tobytes() for t in runner.occupancy_buffers()], losses=losses, spec=dict(runner.speculation_counters()),
               taken=int(runner.votes_off_main_steps))
    del runner
    return out


def test_votes_off_main_steps_equal_the_fused_launches_on_the_emulator(rt, fox_state):
    for depth in (1, 3):
        tail, fused = run_steps(rt, fox_state, 1, depth), run_steps(rt, fox_state, 0, depth)
        # iterations 0 and 5 compact, 7 subdivides: they keep the fused launches; the other six take the tail stream
        assert fused["taken"] == 0 and tail["taken"] == ITERS - 3, (depth, tail["taken"])
        assert tail["losses"] == fused["losses"] and all(x == x for x in tail["losses"]), depth
        for k, (a, b) in enumerate(zip(tail["states"], fused["states"])):
            assert a == b, "depth %d: state tensor %d differs" % (depth, k)
        assert tail["nodes"] == fused["nodes"] and tail["occ"] == fused["occ"], depth
        assert tail["spec"] == fused["spec"], (depth, tail["spec"], fused["spec"])
    # knob 2: the two-deep regime keeps the fused launches
    assert run_steps(rt, fox_state, 2, 3)["taken"] == 0 and run_steps(rt, fox_state, 2, 1)["taken"] == ITERS - 3


def test_no_wait_on_an_unrecorded_event_with_the_votes_on_the_tail_stream(emul_host):
    """(Says something only behind the test above, which runs the steps in this process: alone it reads a counter nobody has touched.
    The pattern of tests/test_wave_emul_cpu.py.)  The stand-in for at::cuda::CUDAEvent counts waits on events nobody has recorded: the tail stream's wait
    for the early stop's event, the side streams' waits for octree_ready_ev_ recorded on the tail stream, the main stream's wait at
    the end of the step."""
    import wemu_build as wave_emul_build
    L = ctypes.CDLL(wave_emul_build.build_host())
    L.wemu_host_unrecorded_waits.restype = ctypes.c_long
    assert L.wemu_host_unrecorded_waits() == 0


# ---- the stream-race detector (tests/wave_emul/stream_races.py) with the knob at 1 ----
# What the comparisons above cannot see -- a stand-in without asynchrony gives the same bytes with a wait missing -- the detector can: it
# keeps the order the host ASKS for (every record / wait as a vector clock per stream) and every global access of every launch.  It
# needs a process of its own (free() that does nothing, so that no address is handed out twice; the traffic build of the kernel
# library under the plain build's soname) and takes most of a minute per scenario: the three scenarios run side by side.
RACE_LINE = re.compile(r"^(read after write|write after read|write after write)\s+(\d+) words\s+(.+?) \[stream (\d+)\]\s+<-\s+(.+?) \[stream (\d+)\]$")
WALK = "(oct_intersect_coop_kernel<2, true>)"  # the speculative walk of a batch sampled ahead (side streams)
# The fused step tail (f2n_field_bwd_step_tail*) runs these three on the tail stream and orders them against the main stream with events
# of the kernel library's own, which the emulator's hipEventRecord / hipStreamWaitEvent stand-ins do not report: the detector lists
# their hand-offs as unordered with the knob at 0 as well (the two-deep scenario).  Not this change's streams or kernels: left out.
STEP_TAIL = ("f2n_reduce_deferred_kernel", "nonfinite_flags_kernel", "adam_fused_kernel")


def parse(text):
    races = [m.groups() for m in map(RACE_LINE.match, text.splitlines()) if m]
    n_said = int(re.search(r"(\d+) distinct \(kernel, kernel, kind\) conflicts", text).group(1))
    assert len(races) == n_said, text  # (every reported line was understood)
    shared = {m.group(2): int(m.group(1)) for m in re.finditer(r"^#     (\d+)  (.+)$", text, re.M)}
    return [(kind, int(n), k2, int(s2), k1, int(s1)) for kind, n, k2, s2, k1, s1 in races], shared


@pytest.fixture(scope="module")
def detector_runs():
    import wemu_build
    wemu_build.build_host()  # (built here, once: the children find both libraries made)
    wemu_build.build(tag="traffic", traffic=True)
    here = os.path.dirname(os.path.abspath(wemu_build.__file__))
    nofree = os.path.join(wemu_build.OUT, "libnofree.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", nofree, os.path.join(here, "nofree.c")], check=True)
    procs = {}
    for name, depth, extra in (("one_ahead", "1", {}), ("two_deep", "3", {}), ("no_waits", "1", {"WEMU_HB_IGNORE_WAITS": "1"})):
        env = dict(os.environ, **extra)
        env["LD_PRELOAD"] = ":".join(x for x in (env.get("LD_PRELOAD", ""), nofree) if x)  # (behind whatever is preloaded already)
        procs[name] = subprocess.Popen([sys.executable, os.path.join(here, "stream_races_votes.py"), "1", "tail", depth], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        text = p.communicate()[0]
        assert p.returncode == 0, text[-3000:]
        print(text)
        out[name] = parse(text)
    return out


@pytest.mark.parametrize("scenario", ["one_ahead", "two_deep"])
def test_stream_race_detector_finds_only_the_designed_pair_with_the_knob_at_one(detector_runs, scenario):
    """Nine emulated training steps (leaves dying under batches sampled ahead, two compactions, a subdivision) with
    ExpRunner.votes_off_main = 1, one batch ahead and two-deep.  The only unordered cross-stream pair is the designed one: the
    speculative walk (side stream) reads node words that the stat update of the running step writes -- on the six eligible steps that
    is update_stats_kernel on the TAIL stream now, on the three maintenance iterations stats_and_scan_kernel on the main stream.
    And the new hand-offs do cross streams and are ordered: words last written by early_stop_kernel (weights, alphas: read by the
    votes on the tail stream), by pack_samples_kernel (bounds, anchors: side stream -> main and tail), by mark_visit_kernel (the vote
    buffer: the next fused launch on the main stream) and by update_stats_kernel (vote rows, stat arrays, node words) are among the
    words touched from more than one stream, and none of them is in an unordered pair but the designed one."""
    races, shared = detector_runs[scenario]
    races = [r for r in races if not ((r[2] in STEP_TAIL and r[3] != 0) or (r[4] in STEP_TAIL and r[5] != 0))]
    assert races, "not even the designed pair: no leaf died under a batch sampled ahead, the scenario checks nothing"
    tail_streams = set()
    for kind, n, second, s2, first, s1 in races:
        assert kind == "write after read" and first == WALK and s1 != 0, (kind, second, s2, first, s1)
        assert (second, s2 == 0) in (("update_stats_kernel", False), ("stats_and_scan_kernel", True)), (second, s2)
        assert s1 != s2
        if second == "update_stats_kernel":
            tail_streams.add(s2)
    assert len(tail_streams) == 1, "the stat update of the eligible steps ran on ONE stream, not the main one: %r" % (races,)
    for writer in ("early_stop_kernel", "pack_samples_kernel", "mark_visit_kernel<true>", "update_stats_kernel"):
        assert shared.get(writer, 0) > 0, "%s wrote nothing that another stream touched: %r" % (writer, shared)


def test_stream_race_detector_sees_the_new_hand_offs_when_no_stream_waits(detector_runs):
    """Positive control (WEMU_HB_IGNORE_WAITS: a host that never makes a stream wait), one batch ahead: what early_stop_ev_ orders --
    the votes on the tail stream behind the early stop's weights / alphas and the sampler's bounds / anchors -- and what the main
    stream's wait for octree_ready_ev_ (JoinTailVotes) orders -- the next fused launches on the main stream behind the tail stream's
    votes and stat update -- are reported, so the test above would notice either wait missing.  (Not seen by this detector: the reuse
    of a freed buffer, since no address is handed out twice; the lifetimes are argued in Renderer.h.)"""
    races, _ = detector_runs["no_waits"]
    pairs = {(kind, second, first) for kind, n, second, s2, first, s1 in races if s1 != s2}
    for want in (("read after write", "mark_visit_kernel<true>", "early_stop_kernel"),
                 ("read after write", "mark_visit_kernel<true>", "pack_samples_kernel"),
                 ("write after write", "early_stop_votes_kernel<true>", "mark_visit_kernel<true>"),
                 ("write after write", "stats_and_scan_kernel", "update_stats_kernel"),
                 ("read after write", "pack_samples_kernel", "update_stats_kernel")):
        assert want in pairs, (want, sorted(pairs))
