"""Option sell_dict_dinv on the host side (no GPU): the public header lists it with its default and its accepted values, the
library's option parser names it with its refusal, and Context.timers() has a slot for the count the GPU tests assert on.
That a context actually refuses other values than 0 and 1 needs a device: tests/test_dict_dinv_gpu.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_option_is_listed_in_the_header_with_its_default():
    text = _read("include", "perphil_hip.h")
    listing = text[text.index("tuning / profiling switches"):]
    assert re.search(r'"sell_dict_dinv" \[1\] \(0 or 1, anything else is refused\)', listing)
    assert listing.index('"sell_dict_zconst" [1]') < listing.index('"sell_dict_dinv" [1]')
    assert "out[35]" in text[:text.index("int pph_get_timers")]


def test_option_parser_refuses_other_values_than_0_and_1():
    src = _read("perphil_amd", "csrc", "pph_api.hip")
    i = src.index('!strcmp(name, "sell_dict_dinv")')
    body = src[i:src.index("return PPH_OK;", i)]
    assert "PPH_REQUIRE(ctx, value == 0.0 || value == 1.0" in body
    assert "la_release_graphs(ctx)" in body       # captured launches carry the kernel choice
    assert _read("perphil_amd", "csrc", "pph_internal.h").count("int sell_dict_dinv = 1;") == 1


def test_timers_report_the_count():
    src = _read("perphil_amd", "_ffi.py")
    assert '"dict_dinv_products": int(t[35])' in src and "np.zeros(36" in src
    api = _read("perphil_amd", "csrc", "pph_api.hip")
    assert "const double v[36]" in api and "i < n && i < 36" in api
