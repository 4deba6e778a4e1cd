"""GPU: the Python glue of `ops.py` makes the calls into the library that tests/golden/ops_call_trace.json.gz recorded
(tools/make_golden_ops_trace.py), call for call and argument for argument.  A change to the glue that is meant to keep what is launched,
in which order and with which arguments - a refactor of the conv + BatchNorm + activation chain or of the head projections - leaves
every case equal; one that is meant to move a launch regenerates the fixture and says so.

Recorded per call: the function and its ints / floats as they are, pointers as null / non-null, ctypes int arrays as their values, ctypes
pointer arrays as their length.  The proxy sits in `yolov10_3d_amd._lib._lib` for the duration of a case and is taken out in a `finally`.

Arms of the glue that the cases reach (checked when the fixture is minted and again in `test_fixture_reaches_every_arm`; the launches
each arm makes are in the trace):
  _stem_forward   fused eval (stem_conv_eval); fused training (stem_conv_train); im2col of a float image and of a uint8 image (NCHW and
                  channels-last) + the dense route
  _dw_forward     eval with BatchNorm + SiLU in the epilogue, without / with a residual (res_mode 1 and 2); eval conv + tail
                  (DW_EVAL_FUSED off); training; the filter pack from the registry and on the spot (PACK_CACHE off)
  _dense_forward  fp8 eval (affine epilogue) and fp8 training; eval affine epilogue; eval affine epilogue with the residual
                  (`conv2d_fwd_affine_res_ok`); eval conv + tail with the residual; training with the pack from the registry (lookup of a
                  new weight, refresh-all after `bump_weight_epoch`) and packed on the spot (PACK_CACHE off, the stem's im2col form)
  _bn_act_tail    training statistics; the pre-BatchNorm hand-over to FusedConvBNProjFn (training); apply with res_mode 0 / 1 / 2; apply that
                  also writes the fp8 copy (bn_act_fwd_q)
  _conv_backward  depth-wise data + weight gradient; fp8 data gradient; bf16 data gradient with the pack from the registry and on the
                  spot; a windowed data gradient (dx_range of the one-to-one head); no data gradient (stem, detached inputs); weight
                  gradient; the stem's dW mapped back
  head glue       HeadProjFn narrow and wide arm, forward and backward (2D head); HeadProjSlicesFn / FusedConvBNProjFn on the VALU forms
                  (16-wide tiny head, PROJ_BN_MFMA off) and on the matrix-core forms (128-wide head); proj_slices_eval on both;
                  conv_bias_act_eval (the model folded the reference's way)
  loss glue       (`loss/...` cases, through the criterion classes of loss.py) Loss3dFn; DualLoss3dFn at an odd element offset; the
                  weighted entry with and without a gradient-pointer array; DistillFn forward, its dense backward (two calls) and the
                  compact rows through the head's slots; Loss2dFn on the dense and on the crowded assigner; FgdmLossFn forward + backward
Not reached: the eval arm of `_bn_act_tail` without `bn_apply` (statistics rows built from the cached scale / shift pair).  Its only
caller, FusedConvBNProjFn, runs in the training forward alone, and the arm makes no launch.
"""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_ops_trace", os.path.join(ROOT, "tools", "make_golden_ops_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()


@pytest.fixture(scope="module")
def recorded():
    return T.load()


def test_fixture_reaches_every_arm(recorded):
    assert list(recorded) == list(T.CASES)
    assert T.unreached(recorded) == []


@pytest.mark.parametrize("case", list(T.CASES))
def test_glue_makes_the_recorded_calls(recorded, case):
    from yolov10_3d_amd import _lib
    before = _lib.lib()
    got = T.run_case(case)
    assert _lib._lib is before, "the recording proxy was left in place"
    diff = T.first_difference(got, recorded[case], context=10)
    if diff:
        print(f"{case}:\n{diff}")
    assert diff is None, f"{case}: the call trace differs from the recorded one (first difference printed above)"
