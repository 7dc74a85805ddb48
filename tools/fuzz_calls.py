"""Random call sequences over every modelled entry point, held to include/pct_hip.h (developer tool): the driver of
tests/test_gpu_call_sequences.py (tests/call_driver.py, the state rules in tests/call_model.py) on fresh seeds for as long
as asked, every profile in turn.  A mismatch prints the seed, the step, the model state and the last eight operations;
call_driver.replay(seed, step, profile) reruns the prefix.  python tools/fuzz_calls.py [seconds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as ge
ge.build()
from point_cloud_toolbox_amd import _capi
import call_driver


def run(seed0=0, budget=60.0, steps=250):
    t_end, seed, done = time.time() + budget, int(seed0), 0
    while time.time() < t_end:
        for profile in call_driver.PROFILES:
            try:
                done += call_driver.run(lambda: _capi.Handle(0), seed, profile, steps)
            except call_driver.Mismatch as e:
                return done, str(e)
            if time.time() >= t_end: break
        seed += 1
    return done, None


if __name__ == "__main__":
    n_done, bad = run(int(sys.argv[2]) if len(sys.argv) > 2 else 0, float(sys.argv[1]) if len(sys.argv) > 1 else 60.0)
    if bad:
        print("MISMATCH", bad, flush=True); sys.exit(1)
    print(f"call fuzz ok: {n_done} steps")
