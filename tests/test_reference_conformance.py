"""Drop-in check of the boundary, without a GPU and without the reference tree.

tests/ref_shaped_model.py builds the residual U-Net through the UN-FUSED MinkowskiEngine surface the reference's own model
files use (MinkowskiConvolution / MinkowskiConvolutionTranspose / MinkowskiBatchNorm constructors with the reference's
keyword arguments and module names).  Built on ``gcl_amd.MinkowskiEngine``, every constructor call must
be accepted, and the resulting parameters must match our own model's names and shapes in both directions (so checkpoints
are interchangeable).  No compute is run here (no GPU)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))        # tests/ref_shaped_model.py

MODEL_KW = dict(bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)


def test_reference_model_builds_on_our_operator_surface():
    import gcl_amd.MinkowskiEngine as ME_amd
    from gcl_amd.model import load_model
    from ref_shaped_model import build
    ref = build(ME_amd, ME_amd.MinkowskiFunctional, 1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5)
    ours = load_model("ResUNetBN2C")(1, 32, **MODEL_KW)
    a, b = ref.state_dict(), ours.state_dict()
    assert list(a.keys()) != [] and set(a.keys()) == set(b.keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) for k in a)
    ours.load_state_dict(a)                       # checkpoints are interchangeable
    ref.load_state_dict(ours.state_dict())
    fat = build(ME_amd, ME_amd.MinkowskiFunctional, 1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5,
                tr_channels=(None, 128, 128, 128, 256))
    assert fat.conv1_tr.kernel.shape == (160, 128)
    fat_ours = load_model("ResUNetFatBN")(1, 32, **MODEL_KW).state_dict()
    fa = fat.state_dict()
    assert set(fa.keys()) == set(fat_ours.keys()) and all(tuple(fa[k].shape) == tuple(fat_ours[k].shape) for k in fa)
