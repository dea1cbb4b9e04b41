"""Census of the reference's probe YAMLs (configs/*.yaml with an ``embedding_dir`` key, the inputs of lp_accel_gpu.py).

    python tools/make_eval_yaml_census.py <reference configs directory>

Writes tests/golden/ref_eval_yaml_census.json: per file the parsed top-level settings, data only.  Paths and wandb names are
dropped (embedding_dir, output_dir, wandb_*); YAML strings stay strings, so the loader's literal decoding (``lr: 1e-4`` is a
YAML string) is exercised by tests/test_lp_cpu.py, which resolves every entry to a probe plan."""
import glob
import json
import os
import sys

import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = {"embedding_dir", "output_dir", "wandb_name", "wandb_job_name", "wandb_account_name"}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    out = {}
    for f in sorted(glob.glob(os.path.join(sys.argv[1], "*.yaml"))):
        d = yaml.safe_load(open(f)) or {}
        if "embedding_dir" not in d:
            continue
        out[os.path.basename(f)] = {"keys": sorted(d), "settings": {k: v for k, v in d.items() if k not in DROP}}
    path = os.path.join(REPO, "tests", "golden", "ref_eval_yaml_census.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(len(out), "probe configs ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
