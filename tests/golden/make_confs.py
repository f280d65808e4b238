"""Records tests/golden/reference_confs.json: the reference's five experiment files (wanjinyou, wanjinyou_big, llff, nerf-360,
free), each composed hydra-style from its `confs/` directory by f2_nerf_amd.config.compose_yaml -- plain key/value settings, the
values f2_nerf_amd.config.PRESETS must equal (tests/test_pipeline_cpu.py::test_presets_equal_the_reference_config_files).

Usage:  python tests/golden/make_confs.py <the reference's confs/ directory>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NAMES = ["wanjinyou", "wanjinyou_big", "llff", "nerf-360", "free"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import config
    out = {name: config.compose_yaml(sys.argv[1], name) for name in NAMES}
    with open(os.path.join(ROOT, "tests", "golden", "reference_confs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
