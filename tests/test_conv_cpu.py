"""CPU-side checks of the conv stage's boundary (osp_conv2d_geometry_t, the output-size rule, the new exports)."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch

from outerspace_amd import _lib
from outerspace_amd import spgemm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_struct_matches_the_header(tmp_path):
    src = tmp_path / "geom.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "outerspace_spgemm.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(osp_conv2d_geometry_t), offsetof(osp_conv2d_geometry_t, dil_w), '
                   'offsetof(osp_conv2d_geometry_t, reserved)); return 0; }\n')
    exe = tmp_path / "geom"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.Conv2dGeometry), _lib.Conv2dGeometry.dil_w.offset, _lib.Conv2dGeometry.reserved.offset]
    assert got == want == [64, 28, 32]


def test_conv_entry_points_are_exported():
    L = _lib.lib()
    for name in ("osp_im2col_csc", "osp_spgemm_conv2d", "osp_csr_maxpool2d"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)


def test_geometry_from_torch_style_arguments():
    g = S.conv2d_geometry((5, 3), stride=2, padding=(1, 0), dilation=(1, 2))
    assert (g.kh, g.kw, g.stride_h, g.stride_w, g.pad_h, g.pad_w, g.dil_h, g.dil_w) == (5, 3, 2, 2, 1, 0, 1, 2)
    assert list(g.reserved) == [0] * 8


def test_output_size_agrees_with_torch():
    """conv2d_output_size against the shape torch's own Unfold gives, over a sweep that includes empty outputs."""
    for size, k, stride, pad, dil in itertools.product((1, 4, 7, 28), (1, 2, 3, 5), (1, 2, 3), (0, 1, 2), (1, 2)):
        got = S.conv2d_output_size(size, k, stride, pad, dil)
        x = torch.zeros(1, 1, size, 1)
        try:
            out = torch.nn.functional.unfold(x, (k, 1), dilation=(dil, 1), padding=(pad, 0), stride=(stride, 1))
            want = out.shape[-1]
        except RuntimeError:   # torch refuses a geometry without output
            want = 0
        assert got == want, (size, k, stride, pad, dil, got, want)


@pytest.mark.parametrize("args", [(28, 5, 1, 2, 1), (14, 5, 1, 0, 1), (10, 2, 2, 0, 1)])
def test_lenet_sizes(args):
    # conv1 keeps 28 x 28, conv2 makes 10 x 10 of 14 x 14, the second pool 5 x 5 of 10 x 10
    want = {28: 28, 14: 10, 10: 5}[args[0]]
    assert S.conv2d_output_size(*args) == want
