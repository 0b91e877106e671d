"""Fixture of the reference's IGDF configs: the parsed contents of its `config/{mujoco,adroit,antmaze}/igdf/*.yaml` files, as data
({domain/env: dict}).  Run where the reference checkout is available:  python tests/golden/make_igdf_config_golden.py"""
import glob
import json
import os

import yaml

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g26_igdf_configs.json")
configs = {}
for domain in ("mujoco", "adroit", "antmaze"):
    for f in sorted(glob.glob(f"/root/reference/config/{domain}/igdf/*.yaml")):
        configs[domain + "/" + os.path.basename(f)[:-len(".yaml")]] = yaml.safe_load(open(f, encoding="utf-8"))
assert len(configs) == 11, sorted(configs)
json.dump(configs, open(OUT, "w"), indent=1, sort_keys=True)
print(sorted(configs), "->", OUT)
