"""GPU: stereo rectification (mlpl_rectify_maps, mlpl_remap_bilinear, mlpl_rectify_images and their device-resident forms) against the
restatement tests/rectify_oracle.py: maps bit for bit, images byte for byte, the fused entry equal to maps followed by remap.  The shapes
are the smallest at which the kernels can go wrong: a lane covers 4 adjacent pixels and a workgroup 256 x 4, so widths 1, 3, 63, 64, 65 and
the 97 x 61 scene cover the vector store, its tail and rows that end inside a lane; 1242 x 375 has more than one workgroup per row."""
import numpy as np
import pytest
import torch

import rectify_oracle as O
import rectify_scenes as S
from matchinglib_poselib_amd import pose
from matchinglib_poselib_amd._lib import MLPL_E_BAD_INPUT, MlplError

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev_maps(ctx, args, w, h, pad=0, offset=0):
    """mlpl_rectify_maps_dev into tensors whose rows are `pad` floats longer than the width and start `offset` floats into their buffer"""
    bx = torch.full((h, w + pad + offset), -7.0, dtype=torch.float32, device="cuda")
    by = torch.full((h, w + pad + offset), -7.0, dtype=torch.float32, device="cuda")
    mx, my = bx[:, offset:offset + w], by[:, offset:offset + w]
    pose.rectify_maps(*args, (w, h), ctx=ctx, device_out=(mx, my))
    torch.cuda.synchronize()
    if pad + offset:   # nothing outside the map was written
        assert (bx[:, :offset] == -7).all() and (bx[:, offset + w:] == -7).all() and (by[:, offset + w:] == -7).all()
    return mx, my


@pytest.mark.parametrize("name", ["small", "strong", "small_resized"])
def test_maps_equal_restatement(ctx, name):
    w, h = S.out_size(name)
    for side in (0, 1):
        ox, oy = S.oracle_maps(name, side)
        gx, gy = pose.rectify_maps(*S.map_args(name, side), (w, h), ctx=ctx)
        assert same_bits(gx, ox) and same_bits(gy, oy), (name, side, "host entry")
        for pad, offset in ((0, 0), (3, 0), (7, 1)):           # the vector store; rows that are not 16-byte aligned
            mx, my = dev_maps(ctx, S.map_args(name, side), w, h, pad, offset)
            assert same_bits(mx.cpu().numpy(), ox) and same_bits(my.cpu().numpy(), oy), (name, side, pad, offset)


@pytest.mark.parametrize("width", [1, 3, 63, 64, 65])
def test_maps_store_tails(ctx, width):
    ox, oy = S.oracle_maps("small", 0, width, 5)
    gx, gy = pose.rectify_maps(*S.map_args("small", 0), (width, 5), ctx=ctx)
    assert same_bits(gx, ox) and same_bits(gy, oy)
    mx, my = dev_maps(ctx, S.map_args("small", 0), width, 5, pad=(4 - width % 4) % 4)
    assert same_bits(mx.cpu().numpy(), ox) and same_bits(my.cpu().numpy(), oy)


def test_maps_one_kitti_image(ctx):
    """more than one workgroup per row and per column"""
    ox, oy = S.oracle_maps("kitti", 1)
    gx, gy = pose.rectify_maps(*S.map_args("kitti", 1), S.out_size("kitti"), ctx=ctx)
    assert same_bits(gx, ox) and same_bits(gy, oy)


def stepped(img, step):
    """the image as rows of `step` bytes (the padding holds 255: reading it would show)"""
    buf = np.full((img.shape[0], step), 255, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def remap_cases():
    cases = {}
    for name, side in (("small", 0), ("small", 1), ("strong", 0), ("small_resized", 1)):
        cases[f"{name}{side}"] = S.oracle_maps(name, side)
    cases["hostile"] = S.hostile_maps(97, 61)
    cases["outside"] = (np.full((6, 13), -40.0, np.float32), np.full((6, 13), 1e4, np.float32))
    for wdt in (1, 3, 63, 64, 65):
        cases[f"w{wdt}"] = S.oracle_maps("small", 0, wdt, 5)
    return cases


@pytest.mark.parametrize("case", sorted(remap_cases()))
def test_remap_equals_restatement(ctx, case):
    """source step 112 for width 97; a hostile value gives 0 and never reaches an address"""
    mx, my = remap_cases()[case]
    img = stepped(S.image(97, 61, 3), 112)
    want = O.remap(img, mx, my)
    assert same_bits(pose.remap_bilinear(img, mx, my, ctx=ctx), want), "host entry"
    if case in ("hostile", "outside"):
        bad = ~np.isfinite(mx) | ~np.isfinite(my) | (np.abs(mx) > 1e6) | (np.abs(my) > 1e6) | (mx < -1) | (my > 62)
        assert bad.sum() >= 30 and not want[bad].any()
    d_img = torch.from_numpy(np.ascontiguousarray(img.base)).cuda()[:, :97]
    h, w = mx.shape
    for pad in (0, 1):                                          # aligned rows with the 4-byte store, unaligned rows with byte stores
        bx = torch.zeros((h, w + pad), dtype=torch.float32, device="cuda")
        by = torch.zeros((h, w + pad), dtype=torch.float32, device="cuda")
        bx[:, :w], by[:, :w] = torch.from_numpy(mx.copy()).cuda(), torch.from_numpy(my.copy()).cuda()
        bo = torch.full((h, w + pad + 2), 9, dtype=torch.uint8, device="cuda")
        out = pose.remap_bilinear(d_img, bx[:, :w], by[:, :w], ctx=ctx, device_out=bo[:, pad:pad + w])
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), want), (case, pad)
        assert (bo[:, :pad] == 9).all() and (bo[:, pad + w:] == 9).all()


def out_of_view_block():
    """a rectifying rotation of 60 degrees about y at a field of view of +-29 degrees: every pixel looks past the image"""
    s = S.SCENES["small"]
    return pose.rectify_param_block(s["K1"], s["dist1"], S.rodrigues((0, 1, 0), 60.0), S.oracle_parameters("small")["Knew"])


def blocks(name):
    return [pose.rectify_param_block(*S.map_args(name, side)) for side in (0, 1)]


def two_step(ctx, d_img, block, w, h):
    """mlpl_rectify_maps_dev followed by mlpl_remap_bilinear_dev"""
    K, dist, Rect, Knew = block[:9], block[9:17], block[17:26], block[26:35]
    mx, my = dev_maps(ctx, (K, dist, Rect, Knew), w, h)
    return pose.remap_bilinear(d_img, mx, my, ctx=ctx)


@pytest.mark.parametrize("new_size", [None, (80, 50), (65, 7)])
def test_fused_equals_maps_then_remap(ctx, new_size):
    """three pairs with three parameter sets in one launch, one of them rotated out of view; also against the restatement"""
    params = np.stack([np.stack(blocks("small")), np.stack(blocks("strong")), np.stack([out_of_view_block(), blocks("strong_partial")[1]])])
    imgs1 = np.stack([stepped(S.image(97, 61, 10 + b), 112).base for b in range(3)])
    imgs2 = np.stack([stepped(S.image(97, 61, 20 + b), 112).base for b in range(3)])
    d1, d2 = torch.from_numpy(imgs1).cuda()[:, :, :97], torch.from_numpy(imgs2).cuda()[:, :, :97]
    w, h = (97, 61) if new_size is None else new_size
    o1, o2 = pose.rectify_images_batch(d1, d2, params, new_size=new_size, ctx=ctx)
    torch.cuda.synchronize()
    for b in range(3):
        for side, (d, o) in enumerate(((d1, o1), (d2, o2))):
            want = two_step(ctx, d[b], params[b, side], w, h)
            torch.cuda.synchronize()
            assert torch.equal(o[b], want), (b, side)
            p = params[b, side]
            mx, my = O.maps(p[:9], p[9:17], p[17:26], p[26:35], w, h)
            assert same_bits(o[b].cpu().numpy(), O.remap(d[b].cpu().numpy(), mx, my)), (b, side, "restatement")
    assert not o1[2].any() and o1[0].any() and o2[2].any()          # the pair that is out of view is black, and only it
    # the single-pair host form
    g1, g2 = pose.rectify_images(imgs1[0][:, :97], imgs2[0][:, :97], params[0], new_size=new_size, ctx=ctx)
    assert same_bits(g1, o1[0].cpu().numpy()) and same_bits(g2, o2[0].cpu().numpy())
    # outputs whose rows are not 4-byte aligned take the byte stores
    bo1 = torch.full((3, h, w + 3), 9, dtype=torch.uint8, device="cuda")
    bo2 = torch.full((3, h, w + 3), 9, dtype=torch.uint8, device="cuda")
    pose.rectify_images_batch(d1, d2, params, new_size=new_size, out=(bo1[:, :, 1:w + 1], bo2[:, :, 1:w + 1]), ctx=ctx)
    torch.cuda.synchronize()
    assert torch.equal(bo1[:, :, 1:w + 1], o1) and torch.equal(bo2[:, :, 1:w + 1], o2)
    assert (bo1[:, :, 0] == 9).all() and (bo1[:, :, w + 1:] == 9).all() and (bo2[:, :, w + 1:] == 9).all()


def test_fused_one_kitti_pair(ctx):
    name = "kitti"
    w, h = S.out_size(name)
    i1, i2 = S.image(w, h, 4), S.image(w, h, 5)
    g1, g2 = pose.rectify_images(i1, i2, np.stack(blocks(name)), ctx=ctx)
    for side, (img, g) in enumerate(((i1, g1), (i2, g2))):
        assert same_bits(g, O.remap(img, *S.oracle_maps(name, side)))
    assert g1.any() and g2.any()


def test_bad_input(ctx):
    def bad(fn):
        with pytest.raises(MlplError) as e:
            fn()
        assert e.value.code == MLPL_E_BAD_INPUT

    a = S.map_args("small", 0)
    img = np.zeros((4, 16385), np.uint8)
    m = np.zeros((2, 2), np.float32)
    bad(lambda: pose.remap_bilinear(img, m, m, ctx=ctx))                                # a side above 16384
    bad(lambda: pose.rectify_maps(*a, (16385, 2), ctx=ctx))
    bad(lambda: pose.rectify_maps(a[0], a[1], a[2], np.full((3, 3), np.nan), (8, 8), ctx=ctx))
    bad(lambda: pose.rectify_maps(a[0], [0.1, 0.2], a[2], a[3], (8, 8), ctx=ctx))
    bad(lambda: pose.remap_bilinear(np.zeros((4, 4), np.float32), m, m, ctx=ctx))
    bad(lambda: pose.rectify_images(np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8), np.stack(blocks("small")), ctx=ctx))
    p = np.stack(blocks("small"))
    p[1, 20] = np.inf
    bad(lambda: pose.rectify_images(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8), p, ctx=ctx))
