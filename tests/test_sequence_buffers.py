"""The buffer plan of a frame sequence (pbrs_amd.api._sequence_buffers) against tables written out by hand from the allocation loop
the plan replaced: names, sizes and their order, for everything on, for the least, and for each option alone."""
from pbrs_amd.api import _sequence_buffers

ALL = ("albedo", "normal", "depth", "instance")

# 16 x 16, guides = ("depth",), nothing else on
LEAST = {"rgb": 3072, "out": 3072, "variance": 1024, "acc_variance": 1024,
         "depth0": 1024, "h_rgb0": 3072, "h_moments0": 2048, "h_length0": 1024,
         "depth1": 1024, "h_rgb1": 3072, "h_moments1": 2048, "h_length1": 1024}
# 16 x 16, all four guides, nothing else on: normal and instance are ping-ponged with the depth, the albedo is single
GUIDED = {"rgb": 3072, "out": 3072, "variance": 1024, "acc_variance": 1024,
          "depth0": 1024, "normal0": 3072, "instance0": 1024, "h_rgb0": 3072, "h_moments0": 2048, "h_length0": 1024,
          "depth1": 1024, "normal1": 3072, "instance1": 1024, "h_rgb1": 3072, "h_moments1": 2048, "h_length1": 1024,
          "albedo": 3072}
MOTION = {"motion": 2048, "prev_depth": 1024}
UPSCALE = {"up": 12288, "albedo_hi": 12288, "normal_hi": 12288, "depth_hi": 4096, "instance_hi": 4096}
DISPLAY_FULL = {"display": 4096, "exposure": 4}


def plan(w=16, h=16, fw=16, fh=16, guides=ALL, motion_vectors=False, upscale=False, display=False):
    return _sequence_buffers(w, h, fw, fh, guides, motion_vectors, upscale, display)


def same(got, want):
    assert list(got.items()) == list(want.items())  # names, sizes and the order they are allocated in


def test_everything_on():
    got = plan(fw=32, fh=32, motion_vectors="prev_depth", upscale=True, display=True)
    same(got, {**GUIDED, **MOTION, **UPSCALE, **DISPLAY_FULL})
    assert len(got) == 26 and sum(got.values()) == 86020
    assert (got["up"], got["normal_hi"], got["depth_hi"], got["display"], got["exposure"], got["h_moments0"], got["albedo"]) == (12288, 12288, 4096, 4096, 4, 2048, 3072)
    assert "albedo0" not in got and "albedo1" not in got


def test_the_least():
    got = plan(guides=("depth",))
    same(got, LEAST)
    assert len(got) == 12 and sum(got.values()) == 22528


def test_each_option_alone():
    same(plan(), GUIDED)
    same(plan(motion_vectors=True), {**GUIDED, **MOTION})
    same(plan(motion_vectors="prev_depth"), {**GUIDED, **MOTION})
    same(plan(display=True), {**GUIDED, "display": 1024, "exposure": 4})                     # at the chain's own size
    same(plan(fw=32, fh=32, upscale=True), {**GUIDED, **UPSCALE})                           # the full-size image and guides only
    same(plan(fw=31, fh=32, upscale=True, guides=("depth",)), {**LEAST, "up": 3 * 31 * 32 * 4, "depth_hi": 31 * 32 * 4})
    same(plan(guides=("depth", "albedo")), {**LEAST, "albedo": 3072})                        # a guide the next frame is not tested against
    same(plan(guides=("normal", "depth")), {**{n: v for n, v in GUIDED.items() if "instance" not in n and n != "albedo"}})
    # the order of `guides` decides the order of the single and the full-size buffers, not of the ping-pong halves
    got = plan(fw=32, fh=32, guides=("instance", "albedo", "depth"), upscale=True)
    assert list(got)[4:8] == ["depth0", "instance0", "h_rgb0", "h_moments0"] and list(got)[-4:] == ["up", "instance_hi", "albedo_hi", "depth_hi"]
    # a film that is not square, and one pixel
    assert plan(w=5, h=3, fw=5, fh=3, guides=("depth",))["h_moments1"] == 2 * 5 * 3 * 4
    assert sum(plan(w=1, h=1, fw=1, fh=1, guides=("depth",)).values()) == 22528 // 256
