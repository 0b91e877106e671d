"""Fixture of the reference's IQL configs: the parsed contents of its four `config/mujoco/iql/*.yaml` files, as data
({env: dict}).  Run where the reference checkout is available:  python tests/golden/make_iql_config_golden.py"""
import glob
import json
import os

import yaml

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g24_iql_configs.json")
configs = {}
for f in sorted(glob.glob("/root/reference/config/mujoco/iql/*.yaml")):
    configs[os.path.basename(f)[:-len(".yaml")]] = yaml.safe_load(open(f, encoding="utf-8"))
assert len(configs) == 4, sorted(configs)
json.dump(configs, open(OUT, "w"), indent=1, sort_keys=True)
print(sorted(configs), "->", OUT)
