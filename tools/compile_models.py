#!/usr/bin/env python3
"""Compile the reference's MJCF robot descriptions into the JSON constant blobs shipped under
dial_mpc_amd/models/ (the XML files themselves are NOT copied into this repository).

Usage (in the build container, where /root/reference is mounted):
    python tools/compile_models.py [--reference /root/reference] [--golden]

--golden also stores every array of the compiled scenes that tests/test_model_compiler.py pins in
tests/golden/mjcf_compiled.npz (keys `<robot>__<scene>__<field>`): the test compares the shipped JSON with
them without needing the XML files.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dial_mpc_amd import mjcf  # noqa: E402

MODELS = [
    ("unitree_go2", "mjx_scene_force.xml"),
    ("unitree_go2", "mjx_scene_force_crate.xml"),
    ("unitree_h1", "mjx_scene_h1_walk.xml"),
    ("unitree_h1", "mjx_scene_h1_loco.xml"),
    ("unitree_h1", "mjx_scene_h1_push_crate.xml"),
    ("wonik_allegro", "scene_left.xml"),
]
# the scenes whose compiled arrays --golden stores (tests/test_model_compiler.py: test_shipped_json_matches_fresh_compile)
GOLDEN_MODELS = [
    ("unitree_go2", "mjx_scene_force.xml"),
    ("unitree_h1", "mjx_scene_h1_walk.xml"),
    ("unitree_go2", "mjx_scene_force_crate.xml"),
    ("unitree_h1", "mjx_scene_h1_push_crate.xml"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--golden", action="store_true", help="also write tests/golden/mjcf_compiled.npz")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_root = os.path.join(root, "dial_mpc_amd", "models")
    for robot, xml in MODELS:
        src = os.path.join(args.reference, "dial_mpc", "models", robot, xml)
        m = mjcf.compile_mjcf(src)
        m["source"] = f"dial_mpc/models/{robot}/{xml}"
        os.makedirs(os.path.join(out_root, robot), exist_ok=True)
        dst = os.path.join(out_root, robot, os.path.splitext(xml)[0] + ".json")
        with open(dst, "w") as f:
            f.write(mjcf.model_to_json(m))
        print(f"{src} -> {dst}  (nq={m['nq']} nv={m['nv']} nu={m['nu']} nbody={m['nbody']} "
              f"ncon={m['ncon']} nefc={m['nefc']})")
    if args.golden:
        import numpy as np
        arrays = {}
        for robot, xml in GOLDEN_MODELS:
            m = mjcf.compile_mjcf(os.path.join(args.reference, "dial_mpc", "models", robot, xml))
            arrays.update({f"{robot}__{os.path.splitext(xml)[0]}__{k}": v for k, v in m.items() if isinstance(v, np.ndarray)})
        dst = os.path.join(root, "tests", "golden", "mjcf_compiled.npz")
        np.savez_compressed(dst, **arrays)
        print(f"{len(arrays)} arrays -> {dst}")


if __name__ == "__main__":
    main()
