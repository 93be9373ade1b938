"""Records tests/golden/launch_trace.json: the sequence of library calls, gradient-ready hooks and gradient destinations that the ops of
dan_amd/ops.py issue for the graphs and configurations of tests/launch_trace.py.

    python tests/golden/make_launch_trace_golden.py [--out tests/golden/launch_trace.json]

RUN THIS AT THE COMMIT BEFORE A CHANGE OF THE GRADIENT HAND-OFF: the file is the behaviour such a change has to reproduce
(tests/test_launch_trace_cpu.py compares the tree under test against it), so it is recorded with dan_amd/ops.py as it was, never from
the code under test.  Nothing is launched and no library is loaded: no GPU and no build are needed.

Layout of the file: "events" is the list of distinct trace entries (tests/launch_trace.py describes them); "traces" maps
"<graph> <configuration>" to the trace as indices into "events", in order.  That is an encoding, not a normalisation: load() gives back
every trace entry by entry.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root (dan_amd)
DEFAULT = os.path.join(HERE, "launch_trace.json")


def encode(traces):
    events, index, out = [], {}, {}
    for key, trace in traces.items():
        ids = []
        for e in trace:
            s = json.dumps(e, separators=(",", ":"), sort_keys=True)
            if s not in index:
                index[s] = len(events)
                events.append(e)
            ids.append(index[s])
        out[key] = ids
    return {"events": events, "traces": out}


def load(path=DEFAULT):
    """{"<graph> <configuration>": trace} as recorded."""
    with open(path) as f:
        g = json.load(f)
    return {key: [g["events"][i] for i in ids] for key, ids in g["traces"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT)
    args = ap.parse_args()
    import launch_trace
    traces = launch_trace.run_all()
    assert launch_trace.run_all() == traces, "the trace is not reproducible"
    g = encode(traces)
    with open(args.out, "w") as f:
        json.dump(g, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d traces, %d entries (%d distinct) -> %s (%d bytes)" % (len(traces), sum(len(t) for t in traces.values()), len(g["events"]), args.out,
                                                                     os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
