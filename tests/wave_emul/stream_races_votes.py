"""Test infrastructure.  The stream-race detector (stream_races.py, same directory: read its text first) with ExpRunner.votes_off_main
set on the runner it makes:
    LD_PRELOAD=_build/libnofree.so python tests/wave_emul/stream_races_votes.py KNOB [the arguments of stream_races.py]
With the knob at 1 the eligible steps of BOTH scenarios (one batch ahead: `tail 1`; two-deep: `tail 3`) cast their votes and update the
statistics on the tail stream.  Driven by tests/test_wave_emul_votes_off_main_cpu.py."""
import sys

import stream_races  # (puts the repository, tests/ and this directory on sys.path)


def main():
    knob = int(sys.argv.pop(1))
    from f2_nerf_amd import runtime
    make_runner = runtime.make_runner

    def make_runner_with_knob(*a, **k):
        made = make_runner(*a, **k)
        made[0].votes_off_main = knob
        return made

    runtime.make_runner = make_runner_with_knob
    return stream_races.main()


if __name__ == "__main__":
    sys.exit(main())
