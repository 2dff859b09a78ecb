"""Fixture generator, run once against a checkout of the reference (`python make_conf_fixture.py <reference checkout>`): the values
of every run config the reference ships (code/confs/**/*.conf) that tests/test_model_cpu.py::test_conf_presets_equal_the_shipped_run_configs
compares with utils/conf.py -- the model subtree, image size, loss block, tracking / mapping loop settings and learning rates ->
tests/golden/reference_confs.json, keyed by the config's path relative to the reference checkout.  Data fixture (numbers and flags), so
that the test runs from the repository alone."""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_confs.json")

MODEL_KEYS = ("implicit_network", "feature_vector_size", "scene_bounding_sphere", "use_warp_loss", "mapping_patchsizes",
              "tracking_patchsizes", "sampling_method", "density_method", "rendering_network", "ray_sampler")
TRACKING_KEYS = ("const_speed_assumption", "lr")
MAPPING_KEYS = ("BA_cam_lr", "keyframe_every", "mapping_every_frame", "mapping_window_size")
TRAIN_KEYS = ("learning_rate", "lr_factor_for_coarse_grid", "lr_factor_for_fine_grid", "lr_factor_for_color_grid",
              "tracking_num_pixels")


def parse_conf(text):
    """the subset of HOCON the shipped run configs use: `name { ... }`, `key = value`, `key = [` ... `]` over several lines"""
    root, stack, lst = {}, [], None
    cur = root
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        if lst is not None:
            if line.startswith("]"):
                lst = None
            else:
                lst.append(_scalar(line))
            continue
        if line.endswith("{"):
            node = {}
            cur[line[:-1].strip()] = node
            stack.append(cur)
            cur = node
        elif line == "}":
            cur = stack.pop()
        elif line.endswith("{}"):
            cur[line[:-2].split("=")[0].strip()] = {}
        else:
            k, v = [t.strip() for t in line.split("=", 1)]
            if v == "[":
                lst = cur[k] = []
            elif v == "[]":
                cur[k] = []
            else:
                cur[k] = _scalar(v)
    return root


def _scalar(v):
    v = v.strip().strip('"')
    if v in ("true", "false"):
        return v == "true"
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


def _pick(d, keys):
    return {k: d[k] for k in keys if k in d}


def extract(conf):
    return {"model": _pick(conf["model"], MODEL_KEYS), "dataset": {"img_res": conf["dataset"]["img_res"]}, "loss": conf["loss"],
            "SLAM": {"tracking": _pick(conf["SLAM"]["tracking"], TRACKING_KEYS), "mapping": _pick(conf["SLAM"]["mapping"], MAPPING_KEYS)},
            "train": _pick(conf["train"], TRAIN_KEYS)}


if __name__ == "__main__":
    REF = sys.argv[1]
    files = sorted(glob.glob(os.path.join(REF, "code", "confs", "**", "*.conf"), recursive=True))
    assert len(files) == 23, len(files)
    out = {os.path.relpath(p, REF): extract(parse_conf(open(p).read())) for p in files}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, len(out))
