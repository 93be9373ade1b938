"""The gradient hand-off of dan_amd/ops.py (GradSlot, gradient sinks, side-stream weight gradients) issues exactly the library calls, hooks
and autograd gradients recorded in tests/golden/launch_trace.json, for every graph and configuration of tests/launch_trace.py: same calls,
same order, same scalar arguments and NULL pattern, same streams.  Host logic only: CPU tensors, no library, no GPU."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import launch_trace  # noqa: E402
import make_launch_trace_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return golden.load()


def test_the_golden_holds_exactly_the_helpers_runs(recorded):
    keys = ["%s %s" % (g, launch_trace.config_key(c)) for g in sorted(launch_trace.GRAPHS) for c in launch_trace.configs()]
    assert len(set(keys)) == len(keys) and sorted(recorded) == sorted(keys)


@pytest.mark.parametrize("graph", sorted(launch_trace.GRAPHS))
def test_launch_trace_is_the_recorded_one(recorded, graph):
    for cfg in launch_trace.configs():
        key = "%s %s" % (graph, launch_trace.config_key(cfg))
        got = json.loads(json.dumps(launch_trace.run(graph, cfg)))          # (tuples -> lists, as the file holds them)
        want = recorded[key]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s: entry %d differs\n  now:      %r\n  recorded: %r" % (key, i, g, w)
        assert len(got) == len(want), "%s: %d entries now, %d recorded" % (key, len(got), len(want))
