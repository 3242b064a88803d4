"""Host: the LDS bank model (tools/lds_banks.py) on the layout conv2 runs with
in the fused conv1+conv2 pipeline: every ds_read_b128 of the 16x16x64 loop,
B fragments (the patch) and A fragments (the resident weights), is
conflict-free, the model still tells the earlier layouts apart, and the LDS
plan fits with the u8 input's table behind it."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def banks():
    spec = importlib.util.spec_from_file_location("lds_banks", os.path.join(ROOT, "tools", "lds_banks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_layout_is_the_kernels(banks):
    """HEADLINE[0] holds the arguments of Conv2Cfg in csrc/conv3x3.hip."""
    src = open(os.path.join(ROOT, "convnet-quantization_amd", "csrc", "conv3x3.hip")).read()
    m = re.search(r"using Conv2Cfg = ConvCfg<([^>]*)>;", src)
    cin, cout, hw, pool, wpx, psp, rpad, spad, split = [a.strip() for a in m.group(1).split(",")]
    name, kw = banks.HEADLINE[0]
    assert name.startswith("conv2")
    assert kw == dict(cin=int(cin), hw=int(hw), pool=pool == "true", wpx=int(wpx), psp=int(psp), rpad=int(rpad),
                      spad=int(spad), split=split == "true", segs=1)
    assert int(cout) == 64
    assert "(4 - ((r >> 2) & 3)) & 3" in src   # res16_swz, as in the model
    assert [banks.res16_swz(r) for r in (0, 4, 8, 12, 17)] == [0, 3, 2, 1, 0]


def test_conv2_b_fragments_conflict_free(banks):
    name, kw = banks.HEADLINE[0]
    assert banks.conflicted(name, kw) == 0
    worst, mean = banks.check(banks.make(name, kw), "16")
    assert (worst, mean) == (4, 4.0)
    # the pixel stride decides it: the Cin + 16 patch is 2-way conflicted for the 16x16 lane groups
    old_name, old_kw = banks.HEADLINE[1]
    assert old_kw["psp"] == 16 and banks.conflicted(old_name, old_kw) == 4 * 8 * 9
    # and any row pad gives the same answer: a 16-pixel block lies in one patch row
    for rpad in (16, 32, 96):
        assert banks.conflicted(name, dict(kw, rpad=rpad)) == 0


def test_conv2_a_fragments_conflict_free(banks):
    assert banks.check_a16(banks.res16_swz) == (4, 4.0)
    assert banks.check_a16(banks.ring_swz)[0] == 8   # the 32x32 loop's swizzle is not


def test_conv12_lds_plan_fits(banks):
    name, kw = banks.HEADLINE[0]
    plan = banks.conv12_lds(banks.make(name, kw))
    assert plan["rows"] == 35 and plan["row_stride"] == 34 * 96
    assert plan["total"] == 161600 and plan["total_u8"] == 162368
    assert plan["total_u8"] <= plan["limit"] == 160 * 1024
    # two whole 18-row patches would not fit
    assert plan["total"] + plan["row_stride"] > plan["limit"]
