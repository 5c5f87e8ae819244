"""Records tests/golden/front_calls_parent.json, on any machine (no GPU): what the composed one-call paths of DeviceSolver --
starts=, bins=, the bootstrap calls, and every refusal -- hand to the library, call by call, for every case of
tests/front_call_cases.py, as this checkout has them.  Run once, on the commit BEFORE those paths were put on one model
binding and one launcher stack; tests/test_front_calls_cpu.py holds every later commit to it.
    python tests/golden/make_front_calls.py [OUT_DIR]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import front_call_cases as FR
    from nonlin_amd import device
    out = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "front_calls_parent.json")
    rec = FR.record_all()
    FR.dump(rec, out)
    assert FR.load(out) == rec                                        # packed without loss
    assert FR.record_all() == rec                                     # and the same on a second run: nothing of this process in it
    calls = [c for v in rec.values() for c in v["trace"]]
    refused = [v for v in rec.values() if "raises" in v]
    print(len(rec), "cases,", len(refused), "refused,", len(calls), "calls of", len({c["entry"] for c in calls}), "entry points,",
          os.path.getsize(out), "bytes, from", device.__file__)
    print("not reached:", sorted(set(FR.REACHABLE) - {c["entry"] for c in calls}),
          "unlisted:", sorted({c["entry"] for c in calls} - set(FR.REACHABLE)))
    for text in sorted({v["raises"] for v in refused}):
        print("  ", text)


if __name__ == "__main__":
    main()
