"""TEST INFRASTRUCTURE — pins what the reference's own constructors build from every shipped yaml (build container only).

    python -m oracle.make_golden_dropin        # writes tests/golden/dropin.json.gz

For each of the twelve `cfg/models/v10/*.yaml` / `cfg/models/v10-3D/*.yaml` the UNPATCHED reference model (oracle/check_dropin.py
`pristine`): `state_dict` keys and shapes, the `save` list, the strides of its host-side probe, the deterministic `bias_init` values,
the output shapes of a train- and an eval-mode forward of a 256x256 probe, and the module paths `BaseModel.fuse()` folds.
tests/test_host_logic.py holds the package's own constructors to it without the reference present.  Data only.
"""
from __future__ import annotations

import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import check_dropin as C  # noqa: E402
from oracle import ref_shim as R  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402


def _plain(o):
    if isinstance(o, tuple):
        return list(o)
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_plain(v) for v in o]
    return o


def main():
    R.import_reference()
    out = {}
    for p in C.yamls():
        info = C.pristine(p)
        out[os.path.basename(p)] = {
            "keys": {k: list(v) for k, v in info["keys"].items()},
            "save": [int(i) for i in info["save"]],
            "stride": [float(s) for s in info["stride"]],
            "bias": {k: [float(x) for x in v.reshape(-1)] for k, v in info["bias"].items()},
            "train_shapes": _plain(info["train_shapes"]),
            "eval_shapes": _plain(info["eval_shapes"]),
            "folded": sorted(info["folded"]),
        }
    path = os.path.join(OUT, "dropin.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:  # mtime 0: same bytes from run to run
        f.write(json.dumps(out, sort_keys=True).encode())
    print(f"{path}: {len(out)} yamls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
