"""The definition of the attention sheets (attngan/attnsheet.py) against the host code it restates, without a
GPU: the table M against miscc/vis.pyramid_expand, the integer blend against Pillow itself over every pair of bytes, the image's byte
against vis._to_uint8_range, and sheet_numpy against what vis.build_super_images2 draws for one sample of five words at 64 -> 256.
The bounds are tests/attnsheet_cases.py's, derived there."""
import numpy as np
import pytest
import torch

import attnsheet_cases as AC
from helpers import load_pkg

load_pkg()
from mogan_amd.attngan import attnsheet as AS  # noqa: E402
from mogan_amd.attngan.miscc import vis  # noqa: E402

TABLES = [(64, 4, 20.0), (128, 2, 20.0), (4, 2, 20.0), (5, 3, 20.0)]


@pytest.mark.parametrize("att,up,sigma", TABLES, ids=str)
def test_the_table_is_the_hosts_upscaling_and_smoothing(att, up, sigma):
    M = AC.table_of(att, up, sigma)
    assert M.shape == (att * up, att) and M.dtype == np.float64
    assert (M >= 0).all()
    assert (np.abs(M.sum(axis=1) - 1.0) <= 4 * AC.EPS).all(), np.abs(M.sum(axis=1) - 1.0).max()
    rng = np.random.RandomState(AC.seed_of("table", (att, up)))
    A = rng.uniform(0, 1, (att, att))
    want = vis.pyramid_expand(A[:, :, None], upscale=up, sigma=sigma)[:, :, 0]
    got = M @ A @ M.T
    err = np.abs(got - want).max() / np.abs(want).max()
    print("table (%d, %d, sigma %g): M A M^T is within %.2e of pyramid_expand's maximum" % (att, up, sigma, err))
    assert err <= 1e-13


def test_the_table_without_upscaling_is_the_identity_exactly():
    for att in (2, 5, 128):
        M = AS.table(att, 1, 20.0)
        assert M.dtype == np.float64 and (M == np.eye(att)).all()
    with pytest.raises(ValueError):
        AS.table(0, 2)
    with pytest.raises(ValueError):
        AS.table(4, 0)


@pytest.mark.parametrize("alpha", [180, 0, 255])
def test_the_integer_blend_is_pillows_paste_for_every_pair_of_bytes(alpha):
    byte = np.arange(256, dtype=np.uint8)
    image = np.repeat(byte[:, None], 256, axis=1)                  # the image's byte down the rows
    level = np.repeat(byte[None, :], 256, axis=0)                  # the map's byte along the columns
    want = vis._blend(np.stack([image] * 3, axis=-1), np.stack([level] * 3, axis=-1), 256, alpha)
    got = AS.blend_u8(image, level, alpha)
    assert got.dtype == np.uint8 and (want == got[:, :, None]).all()


def test_the_images_byte_is_the_hosts():
    rng = np.random.RandomState(AC.seed_of("byte", 0))
    x = np.clip(rng.standard_normal((2, 3, 256, 256)) * 0.7, -1, 1).astype(np.float32)
    x[0, 0, 0, :4] = (-1.0, 1.0, 0.0, np.nextafter(np.float32(1), np.float32(0)))
    want = np.uint8(vis._to_uint8_range(torch.from_numpy(x), 256))                           # (B, vis, vis, 3)
    assert (AS.image_u8(x).transpose(0, 2, 3, 1) == want).all()
    wild = np.array([-3.0, 2.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    assert AS.image_u8(wild).tolist() == [0, 255, 0, 255, 0]


def test_the_sheet_is_what_the_host_function_draws():
    """one sample of five words at 64 -> 256: the blended images of build_super_images2 in its own top-K order"""
    key = (5, 5, 64, 4)
    att, vis_size, T = 64, 256, 5
    lens = np.array([T], dtype=np.int32)
    attn = AC.attention(key, lens, "host function")
    img = AC.image(key, 1)
    M = AC.table_of(att, 4, 20.0)
    conf = AS.conf_numpy(attn, lens)
    order = AS.top_words(conf[0], T, 5)
    pick = np.array([(0, w) for w in order], dtype=np.int32)
    e = AC.expected_of(attn, lens, img, M, pick)
    assert (e["flags"] == 0).all()
    captions = torch.arange(1, T + 1)[None]
    ixtoword = {i: "w%d" % i for i in range(T + 1)}
    drawn, _ = vis.build_super_images2(torch.from_numpy(img), captions, lens, ixtoword, [torch.from_numpy(attn[0])], att, vis_size, topK=5)
    assert drawn.shape == (vis.FONT_MAX + vis_size, 5 * (vis_size + 2), 3)
    host = np.stack([drawn[vis.FONT_MAX:, i * (vis_size + 2):i * (vis_size + 2) + vis_size] for i in range(5)])
    # the host orders by its conf_score, three times conf in fp32 (its channels are repeated): sheet i is word order[i] only if both agree
    n = AC.check_sheet(host, e, "sheet_numpy against build_super_images2")
    print("%d of %d pixels one level apart" % (n, 5 * vis_size * vis_size))


def test_the_oracle_answers_the_picks_that_are_never_sent_and_the_flat_map():
    key = (4, 3, 2, 2)
    attn, lens, img, M, pick = AC.case(key)
    B, T = attn.shape[:2]
    bad = np.array([(-1, 0), (B, 0), (1, T), (2, int(lens[2])), (0, 0)], dtype=np.int32)
    sheet, stats, flags = AS.sheet_numpy(attn, lens, img, M, bad)
    assert flags.tolist() == [AS.NEVER] * 4 + [AS.FLAT]
    assert not sheet[:4].any() and not stats.any()
    assert (sheet[4] == AS.blend_u8(AS.image_u8(img[0]).transpose(1, 2, 0), np.zeros((4, 4, 1), dtype=np.uint8))).all()
    hot = attn.copy()
    hot[1, 0, 0, 0] = np.inf
    assert AS.sheet_numpy(hot, lens, img, M, np.array([(1, 0)], dtype=np.int32))[2].tolist() == [AS.NONFINITE]
    attn, lens = AC.case((4, 9, 16, 2))[:2]                      # 4 / len < 1 only from four words on
    conf = AS.conf_numpy(attn, lens)
    assert (conf[0] == 0).all() and (conf[2, int(lens[2]):] == 0).all() and (conf[1] > 0).all() and (conf[2, :int(lens[2])] > 0).all()
