"""Record how often every mixture-of-experts layer calls each entry point of the library in one forward + backward.

    python tools/record_moe_launches.py [--out tests/golden/moe_launches.json]

Runs the cases of ``tests/test_moe_segmented_gpu.py`` (``LAUNCH_CASES``: LatentMoE A and B, classic MoE A and B, one DeepSeekMoE layer, Qwen3MoE at
E = 8, each on the segmented and on the per-expert path) through the layers' public modules and writes {case: {path: {entry point: calls}}}.  The test
``test_every_layer_issues_the_recorded_launches`` holds the host layer to this record, so it is written from the commit BEFORE a change that must not
alter the launches.  Needs the GPU.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "moe_launches.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_moe_launches.py needs an MI355X: the launches are counted on a real forward + backward")
    import test_moe_segmented_gpu as T

    record = {case: {path: T.launch_counts(case, on) for path, on in T.PATHS.items()} for case in T.LAUNCH_CASES}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    for case, paths in record.items():
        print(case, {path: sum(c.values()) for path, c in paths.items()})


if __name__ == "__main__":
    main()
