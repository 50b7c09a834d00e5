"""The float tolerances of tests/test_wrappers_fused.py, measured on the TENSOR wrapper stack (so: from the code as it stood before the fused kernels existed).
    python tests/tools/wrappers_fused_spread.py          writes tests/golden/wrappers_fused_spread.json
golden:  per golden file and key, the largest distance of the tensor stack fed fp32 inputs (CPU) from the golden's fp64 values over the replay.
twin:    per key of the twin protocol (per-env-distinct scripted envs, B = 5 and B = 130), the distance of the fp32 tensor stack from the same stack fed the
         same numbers as fp64.
The fused path gets 3 x that per key (the rule of tests/golden/ycb_pair_spread.json), at least 3 fp32 ulps at the key's largest magnitude in the protocol.
Also prints the threshold margin of the twin test's seed: no draw of the protocol may lie within 4 fp32 ulps of the threshold it is compared with."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_wrappers_fused as T  # noqa: E402
from robogym_amd.envs.dactyl.locked import load_locked_model  # noqa: E402


def main():
    model = load_locked_model()
    out = {"rule": "tolerance = max(3 x yardstick distance, 3 fp32 ulps at the key's largest magnitude)", "twin_seed": T.TWIN_SEED, "golden": {}, "yardstick": {"golden": {}}}
    for name, W in (("wrappers_randomized", T.randomized_golden_replay(model, None, "fp32")), ("wrappers", T.plain_golden_replay("wrappers", model, None, "fp32")),
                    ("wrappers_fixed_wrist", T.plain_golden_replay("wrappers_fixed_wrist", model, None, "fp32", fixed_wrist=True))):
        out["golden"][name] = T.tolerances(W)
        out["yardstick"]["golden"][name] = W.dist
    W = T.Worst()
    for B in (5, 130):
        fp32, margin = T.twin_rollout(model, B, "cpu", None, "fp32")
        fp64, _ = T.twin_rollout(model, B, "cpu", None, "fp64")
        T.compare_twin(fp32, fp64, W)
        print("twin seed %d, B = %d: smallest threshold margin %.1f fp32 ulps (must exceed 4)" % (T.TWIN_SEED, B, margin))
        assert margin > 4.0
    out["twin"] = T.tolerances(W)
    out["yardstick"]["twin"] = W.dist
    with open(T.SPREAD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for sect in ("golden", "twin"):
        print(sect, json.dumps(out[sect], sort_keys=True)[:600], "...")


if __name__ == "__main__":
    main()
