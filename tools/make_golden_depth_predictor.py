"""Mints tests/golden/depth_predictor.npz from the REFERENCE's `DepthPredictor` (nn/modules/head.py:978-1042), run on the CPU in float32:

    python tools/make_golden_depth_predictor.py      # needs the reference checkout (oracle.ref_shim.REF_ROOT)

For every case of tests/depth_predictor_ref.py (`CASES`) the reference module is built under `torch.manual_seed(SEED)`, its GroupNorm
affine pairs are redrawn (`redraw_affine`), and it runs `forward(features, return_embeddings=True)` and the backward of
sum(logits * cotangent) through torch.autograd.  The inputs are not stored: the features and the cotangent are drawn from the case's seed
(`case_inputs`), the parameters are rebuilt from the seed by the test.  The file records results only, and EVERY tensor is sampled: per
case `<name>/<key>/sum` (float64 sum of the float32 tensor) and `<name>/<key>/sample` = flat[::ceil(numel / SAMPLES)] (float32), for
  p_<state_dict key>   every parameter as built (the test's own module must reproduce them: same draws in the same order),
  logits, weighted_depth, features,
  d_feat0 .. d_feat2, d_<state_dict key>   the gradients wrt the three features and every trainable parameter.
Tensors of at most SAMPLES values are therefore stored whole; the two 128 x 128 x 3 x 3 weights (147 456 values each) and the S-3D case's
maps are the ones a sample stands for."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_predictor_ref as R  # noqa: E402
from oracle import ref_shim  # noqa: E402


def main():
    ref_shim.import_reference()
    from ultralytics.nn.modules.head import DepthPredictor
    out = {}
    for case in R.CASES:
        torch.manual_seed(R.SEED)
        m = R.redraw_affine(DepthPredictor(case["ch"])).train()
        feats, cot = R.case_inputs(case)
        feats = [f.requires_grad_(True) for f in feats]
        logits, weighted, features = m(feats, return_embeddings=True)
        (logits * cot).sum().backward()
        rec = {"logits": logits, "weighted_depth": weighted, "features": features}
        rec.update({f"d_feat{i}": f.grad for i, f in enumerate(feats)})
        for k, v in m.state_dict().items():
            rec[f"p_{k}"] = v
        for k, v in m.named_parameters():
            if v.requires_grad:
                rec[f"d_{k}"] = v.grad
        for k, v in rec.items():
            a = v.detach().numpy()
            assert a.dtype == np.float32
            out[f"{case['name']}/{k}/sum"] = np.float64(a.astype(np.float64).sum())
            out[f"{case['name']}/{k}/sample"] = R.sample(a).astype(np.float32)
        print(f"{case['name']}: {len(rec)} tensors")
    np.savez_compressed(R.GOLDEN, **out)
    print(f"wrote {R.GOLDEN} ({os.path.getsize(R.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
