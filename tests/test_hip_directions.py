"""Direction search on the GPU: ch_sheet_compose and ch_sweep_stats bit for bit against the numpy oracles (tests/sheet_oracle.py),
DirectionSearch's sweeps, sheets and job files, and Backend.sweep_direction against the per-value API."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ctrlhair_amd import directions as DS
from ctrlhair_amd import hostutil as U
from ctrlhair_amd import lib as L
from ctrlhair_amd import procedural as P
from tests import sheet_oracle as SO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
NGF = 16      # tiny SEAN generator, as tests/test_backend.py; the other networks are full size

# x * 127.5 + 127.5 gives another byte when fused (tests/test_directions.py::test_unfused_conversion_values), then the range's ends
SPECIAL = [float.fromhex(h) for h in ('-0x1.676768p-1', '-0x1.31313ap-4', '-0x1.575758p-1', '-0x1.bfbfc0p-1', '-0x1.c5c5c8p-2',
                                      '-0x1.11111ap-4')] + [1.0, -1.0, 1.5, -1.5, float('nan'), float('inf'), float('-inf')]


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


def _sources(kind, n, Hs, Ws, seed):
    rng = np.random.default_rng(seed)
    if kind == 0:
        a = rng.uniform(-1.2, 1.2, (n, 3, Hs, Ws)).astype(np.float32)
        a.reshape(-1)[:len(SPECIAL)] = SPECIAL
        a[-1].reshape(-1)[-len(SPECIAL):] = SPECIAL
        return a
    if kind == 1:
        return rng.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (n, Hs, Ws), dtype=np.uint8)
    lab.reshape(-1)[:6] = [19, 200, 254, 255, 13, 0]                         # beyond the 19 classes: black, and 255: white
    return lab


def _scrambled_cells(rows, cols, n, seed):
    order = np.random.default_rng(seed).permutation(rows * cols)[:n]
    return [(int(k) // cols, int(k) % cols) for k in order]


@pytest.mark.parametrize('margin', [0, 1, 5])
@pytest.mark.parametrize('cell', [(7, 5), (12, 20), (16, 16), (256, 256)])
def test_compose_equals_the_oracle(handle, cell, margin):
    H, W = cell
    rows, cols = (3, 4) if H < 256 else (2, 2)
    for kind in (0, 1, 2):
        for n in range(1, rows * cols + 1):
            src = _sources(kind, n, H, W, seed=100 * kind + n)
            cells = _scrambled_cells(rows, cols, n, seed=n + margin)
            sheet = DS.ContactSheet(handle, 'cuda:0', rows, cols, cell, margin)
            sheet.draw(torch.from_numpy(src).cuda(), cells, draw_type=2 if kind == 2 else None)
            want = np.full((rows * H, cols * W + margin * (cols - 1), 3), 255, np.uint8)
            SO.compose(want, src, kind, cells, rows, cols, H, W, margin, lut=DS.mask_lut(2))
            got = sheet.numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (kind, n, cells)
            if n < rows * cols or margin:
                assert (want == 255).all(axis=2).any()                       # untouched cells / margins are part of the comparison


def test_compose_skips_a_cell_outside_the_grid(handle):
    rows, cols, H, W, margin = 2, 3, 12, 20, 1
    for bad in ((rows, 0), (0, cols), (-1, 1), (1, -1)):
        src = _sources(1, 3, H, W, seed=7)
        cells = [(1, 2), bad, (0, 0)]
        canvas = torch.full((rows * H, cols * W + margin * (cols - 1), 3), 255, dtype=torch.uint8, device='cuda')
        pad = torch.full((4096,), 77, dtype=torch.uint8, device='cuda')      # (whatever lies around is left alone too)
        s, c = torch.from_numpy(src).cuda(), torch.tensor(cells, dtype=torch.int32, device='cuda')
        handle.call('ch_sheet_compose', s.data_ptr(), 1, 3, H, W, c.data_ptr(), None, canvas.data_ptr(), rows, cols, H, W, margin, None)
        want = np.full(tuple(canvas.shape), 255, np.uint8)
        SO.compose(want, src, 1, cells, rows, cols, H, W, margin)
        assert np.array_equal(U.to_host(canvas), want) and (want[H:, :W] == 255).all() and bool((pad == 77).all())
        with pytest.raises(ValueError):
            DS.ContactSheet(handle, 'cuda:0', rows, cols, (H, W), margin).draw(s, cells)     # the wrapper refuses it before upload


@pytest.mark.parametrize('src_size,cell,kinds', [((8, 10), (16, 20), (0, 1, 2)), ((256, 256), (512, 512), (2,)), ((16, 20), (7, 5), (0, 2))])
def test_compose_nearest_maps_other_sizes(handle, src_size, cell, kinds):
    (Hs, Ws), (H, W) = src_size, cell
    rows, cols, margin = 1, 2, 3
    for kind in kinds:
        src = _sources(kind, 2, Hs, Ws, seed=kind)
        cells = [(0, 1), (0, 0)]
        for draw_type in ((1, 2) if kind == 2 else (None,)):
            sheet = DS.ContactSheet(handle, 'cuda:0', rows, cols, cell, margin).draw(torch.from_numpy(src).cuda(), cells, draw_type=draw_type)
            want = np.full((rows * H, cols * W + margin, 3), 255, np.uint8)
            SO.compose(want, src, kind, cells, rows, cols, H, W, margin, lut=DS.mask_lut(draw_type) if kind == 2 else None)
            assert np.array_equal(sheet.numpy(), want), (kind, draw_type)


def test_two_draws_on_one_canvas(handle):
    I, V, S, margin = 3, 2, 16, 2
    imgs, masks = _sources(0, I * V, S, S, seed=1), _sources(2, I * V, 8, 8, seed=2)
    img_cells = [(2 * i, v) for i in range(I) for v in range(V)]
    mask_cells = [(2 * i + 1, v) for i in range(I) for v in range(V)]
    sheet = DS.ContactSheet(handle, 'cuda:0', 2 * I, V, S, margin)
    sheet.draw(torch.from_numpy(imgs).cuda(), img_cells).draw(torch.from_numpy(masks).cuda(), mask_cells, draw_type=2)
    want = np.full((2 * I * S, V * S + margin, 3), 255, np.uint8)
    SO.compose(want, imgs, 0, img_cells, 2 * I, V, S, S, margin)
    SO.compose(want, masks, 2, mask_cells, 2 * I, V, S, S, margin, lut=DS.mask_lut(2))
    assert np.array_equal(sheet.numpy(), want)


def _renders(N, H, W, h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.1, 1.1, (N, 3, H, W)).astype(np.float32)
    img.reshape(-1)[:len(SPECIAL)] = SPECIAL
    lab = rng.choice(np.array([13, 13, 1, 2, 17, 255], np.uint8), size=(N, h, w))
    lab[N // 2] = 13                                                         # all hair
    if N > 1:
        lab[N - 1][lab[N - 1] == 13] = 4                                     # no hair
    return img, lab


def _measure_both_kinds(handle, img, lab, ref):
    st = DS.SweepStats(handle, 'cuda:0')
    lab_d = torch.from_numpy(lab).cuda()
    got0 = U.to_host(st.measure(torch.from_numpy(img).cuda(), lab_d, ref))
    u8 = np.ascontiguousarray(SO.to_u8(img).transpose(0, 2, 3, 1))
    got1 = U.to_host(st.measure(torch.from_numpy(u8).cuda(), lab_d, ref))
    return got0, got1, u8


@pytest.mark.parametrize('N', [1, 7, 60])
@pytest.mark.parametrize('size', [(5, 7), (16, 16), (64, 48), (256, 256)])
def test_sweep_stats_equal_the_oracle(handle, N, size):
    H, W = size
    img, lab = _renders(N, H, W, H, W, seed=N + H)
    V = 6
    ref = np.array([n if n % 3 == 0 else (-1 if n % 3 == 1 else (n // V) * V) for n in range(N)])    # itself, none, the row's start
    got0, got1, u8 = _measure_both_kinds(handle, img, lab, ref)
    want = SO.sweep_stats(u8, 1, lab, ref)
    assert got0.dtype == np.int64 and got0.shape == (N, 16)
    assert np.array_equal(got0, want) and np.array_equal(got1, want)
    assert want[N // 2, 0] == H * W and (N == 1 or (want[N - 1, 5:9] == -1).all())
    assert not want[ref < 0, 12:].any() and not want[ref == np.arange(N)][:, [12, 14]].any()
    again = U.to_host(DS.SweepStats(handle, 'cuda:0').measure(torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), ref))
    assert np.array_equal(again, got0)                                       # integer atomics: the same array every time


@pytest.mark.parametrize('mode', ['self', 'none', 'row'])
def test_sweep_stats_reference_modes(handle, mode):
    N, V = 12, 6
    img, lab = _renders(N, 16, 16, 16, 16, seed=3)
    ref = {'self': np.arange(N), 'none': np.full(N, -1), 'row': (np.arange(N) // V) * V}[mode]
    got0, got1, u8 = _measure_both_kinds(handle, img, lab, ref)
    want = SO.sweep_stats(u8, 1, lab, ref)
    assert np.array_equal(got0, want) and np.array_equal(got1, want)
    if mode == 'self':
        assert not want[:, [12, 14]].any() and np.array_equal(want[:, 13], want[:, 0]) and np.array_equal(want[:, 15], want[:, 0])
    if mode == 'none':
        assert not want[:, 12:].any()
    if mode == 'row':
        assert want[1:V, 12].all() and want[N - 1, 15] == want[V, 0]            # the last render has no hair: the union is the reference's
    dev_ref = torch.from_numpy(ref.astype(np.int32)).cuda()                 # a device array is passed through
    assert np.array_equal(U.to_host(DS.SweepStats(handle, 'cuda:0').measure(torch.from_numpy(u8).cuda(), torch.from_numpy(lab).cuda(),
                                                                             dev_ref)), want)


def test_sweep_stats_label_maps_at_half_size(handle):
    img, lab = _renders(3, 512, 512, 256, 256, seed=9)                       # render 1 all hair, render 2 none
    ref = np.array([-1, 0, 1])
    got0, got1, u8 = _measure_both_kinds(handle, img, lab, ref)
    want = SO.sweep_stats(u8, 1, lab, ref)
    assert np.array_equal(got0, want) and np.array_equal(got1, want)
    assert want[1, 0] == 512 * 512 and (want[2, 5:9] == -1).all() and want[2, 15] == 512 * 512


def test_argument_errors_name_the_function(handle):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()

    def raw(fn, *args):
        rc = getattr(handle.lib, fn)(handle._h, *args)
        return rc, handle.lib.ch_last_error(handle._h).decode()

    good = dict(src=p, kind=1, n=1, Hs=4, Ws=4, cells=p, lut=p, canvas=p, rows=1, cols=1, H=4, W=4, margin=0)
    for change in (dict(src=None), dict(cells=None), dict(canvas=None), dict(kind=2, lut=None), dict(kind=3), dict(kind=-1), dict(n=0),
                   dict(n=65536), dict(Hs=0), dict(Ws=-1), dict(rows=0), dict(cols=0), dict(H=0), dict(W=0), dict(margin=-1)):
        a = dict(good, **change)
        rc, msg = raw('ch_sheet_compose', a['src'], a['kind'], a['n'], a['Hs'], a['Ws'], a['cells'], a['lut'], a['canvas'], a['rows'],
                      a['cols'], a['H'], a['W'], a['margin'], None)
        assert rc == ERR_ARG and 'ch_sheet_compose' in msg, (change, rc, msg)
    good = dict(img=p, kind=1, labels=p, ref=p, N=1, H=4, W=4, h=4, w=4, stats=p)
    for change in (dict(img=None), dict(labels=None), dict(ref=None), dict(stats=None), dict(kind=2), dict(N=0), dict(N=65536), dict(H=0),
                   dict(W=0), dict(h=0), dict(w=-3), dict(H=40000)):
        a = dict(good, **change)
        rc, msg = raw('ch_sweep_stats', a['img'], a['kind'], a['labels'], a['ref'], a['N'], a['H'], a['W'], a['h'], a['w'], a['stats'], None)
        assert rc == ERR_ARG and 'ch_sweep_stats' in msg, (change, rc, msg)
    assert not bool(buf.any())                                               # nothing was launched
    st = DS.SweepStats(handle, 'cuda:0')
    img, lab = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device='cuda'), torch.zeros(2, 4, 4, dtype=torch.uint8, device='cuda')
    for ref in ([0, 2], [-2, 0], [0]):
        with pytest.raises(ValueError):
            st.measure(img, lab, ref)                                        # a reference the wrapper can see is out of range


# ---- DirectionSearch ----------------------------------------------------------------------------------------------------------
def _weights():
    from ctrlhair_amd.hair_editor import procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, NGF)
    return w


I_IMGS, VALUES = 2, [-2.5, 0.0, 2.5]


@pytest.fixture(scope='module')
def search(hip_lib):
    from ctrlhair_amd.pipeline import EditPipeline
    pipe = EditPipeline(_weights(), device=0, img_size=256, max_batch=4)     # 6 renders per candidate: chunks of 4 + 2
    imgs = torch.from_numpy(P.synthetic_images(I_IMGS, 256, seed=3)).cuda()
    yield DS.DirectionSearch(pipe, imgs, noise_seed=5)
    pipe.close()


def _oracle_sheet(search, att, images, masks, cell=256):
    I, V = images.shape[:2]
    step = 2 if att == 'shape' else 1
    rows, cols = step * I, V + 1
    want = np.full((rows * cell, cols * cell, 3), 255, np.uint8)
    imgs_in, im, mk = U.to_host(search.imgs), U.to_host(images), U.to_host(masks)
    SO.compose(want, imgs_in, 0, [(step * i, 0) for i in range(I)], rows, cols, cell, cell, 0)
    SO.compose(want, im.reshape(I * V, *im.shape[2:]), 0, [(step * i, v + 1) for i in range(I) for v in range(V)], rows, cols, cell, cell, 0)
    if att == 'shape':
        SO.compose(want, U.to_host(search.input_masks), 2, [(2 * i + 1, 0) for i in range(I)], rows, cols, cell, cell, 0, lut=DS.mask_lut(1))
        SO.compose(want, mk.reshape(I * V, 256, 256), 2, [(2 * i + 1, v + 1) for i in range(I) for v in range(V)], rows, cols, cell, cell, 0,
                   lut=DS.mask_lut(2))
    return want


def test_texture_sweep_and_sheet(search):
    d = DS.candidate_direction(8, [], 0, 0)
    images, masks = search.sweep('texture', d, VALUES)
    assert tuple(images.shape) == (I_IMGS, 3, 3, 256, 256) and tuple(masks.shape) == (I_IMGS, 3, 256, 256)
    assert bool((masks == search.input_masks[:, None]).all())               # the input's decoded mask, every value
    st = search.stats(images, masks)
    assert st.shape == (I_IMGS, 3, 16) and not st[:, :, 12].any()            # a texture move changes no label
    assert (st[:, 1:, 14] > 0)[st[:, 1:, 15] > 0].all()                      # ... but it does change the hair's pixels, where there are any
    moved = search.latents('texture', d, VALUES)
    assert float(((moved @ d.cuda()) - torch.tensor(VALUES, device='cuda')).abs().max()) <= 1e-5
    assert np.array_equal(search.sheet('texture', images, masks).numpy(), _oracle_sheet(search, 'texture', images, masks))
    sc = DS.score('texture', st, VALUES, 256, 256)
    assert (sc['effect'] > 0) == bool(st[:, -1, 15].any()) and 0 <= sc['monotone'] <= 1


def test_shape_sweep_and_sheet(search):
    d = DS.candidate_direction(16, [], 0, 1)
    images, masks = search.sweep('shape', d, VALUES)
    st = search.stats(images, masks)
    assert st[:, -1, 12].all() and not st[:, 0, [12, 14]].any()              # the masks move; the first value is its own reference
    assert np.array_equal(st, SO.sweep_stats(U.to_host(images).reshape(-1, 3, 256, 256), 0, U.to_host(masks).reshape(-1, 256, 256),
                                             np.repeat(np.arange(I_IMGS) * 3, 3)).reshape(I_IMGS, 3, 16))
    got = search.sheet('shape', images, masks).numpy()
    assert got.shape == (2 * I_IMGS * 256, 4 * 256, 3)
    assert np.array_equal(got, _oracle_sheet(search, 'shape', images, masks))
    # smaller cells: the uint8 images through ch_resize_linear_u8, label maps nearest-mapped
    small = search.sheet('shape', images, masks, cell=64).numpy()
    want = np.full((2 * I_IMGS * 64, 4 * 64, 3), 255, np.uint8)
    r = lambda x: U.to_host(search.resizer.resize(DS.to_u8(x), 64))
    cells = [(2 * i, v + 1) for i in range(I_IMGS) for v in range(3)]
    SO.compose(want, r(search.imgs), 1, [(2 * i, 0) for i in range(I_IMGS)], 2 * I_IMGS, 4, 64, 64, 0)
    SO.compose(want, r(images.reshape(-1, 3, 256, 256)), 1, cells, 2 * I_IMGS, 4, 64, 64, 0)
    SO.compose(want, U.to_host(search.input_masks), 2, [(2 * i + 1, 0) for i in range(I_IMGS)], 2 * I_IMGS, 4, 64, 64, 0, lut=DS.mask_lut(1))
    SO.compose(want, U.to_host(masks).reshape(-1, 256, 256), 2, [(r_ + 1, c) for r_, c in cells], 2 * I_IMGS, 4, 64, 64, 0, lut=DS.mask_lut(2))
    assert np.array_equal(small, want)


def test_job_files_do_not_depend_on_the_sharding(search, tmp_path):
    from PIL import Image
    one, two = str(tmp_path / 'one'), str(tmp_path / 'two')
    recs = DS.find_directions(search, 'shape', [], one, n=4, values=VALUES, seed=2, rank=0, world=1)
    for rank in (0, 1):
        DS.find_directions(search, 'shape', [], two, n=4, values=VALUES, seed=2, rank=rank, world=2)
    assert sorted(r['index'] for r in recs) == [0, 1, 2, 3]
    for i in range(4):
        for rel in (os.path.join('shape_dir_1', f'{i}.pkl'), os.path.join('shape_1', f'{i}.png')):
            with open(os.path.join(one, rel), 'rb') as f, open(os.path.join(two, rel), 'rb') as g:
                assert f.read() == g.read(), rel
    merged = DS.merge_scores(one)
    assert merged == DS.merge_scores(two, world=2) and len(merged) == 4
    assert [m['effect'] for m in merged] == sorted((m['effect'] for m in merged), reverse=True)
    # the PNG is the sheet
    d = DS.candidate_direction(16, [], 2, 3)
    assert np.array_equal(d.numpy(), DS.load_used(os.path.join(one, 'shape_dir_1'))[3])
    images, masks = search.sweep('shape', d, VALUES)
    png = np.asarray(Image.open(os.path.join(one, 'shape_1', '3.png')).convert('RGB'))
    assert np.array_equal(png, search.sheet('shape', images, masks).numpy())
    # top:K renders only the best K of the rank again
    three = str(tmp_path / 'three')
    top = DS.find_directions(search, 'shape', [], three, n=4, values=VALUES, seed=2, sheets='top:1')
    assert top == recs and os.listdir(os.path.join(three, 'shape_1')) == ['%d.png' % merged[0]['index']]
    with open(os.path.join(three, 'shape_1', '%d.png' % merged[0]['index']), 'rb') as f, \
            open(os.path.join(one, 'shape_1', '%d.png' % merged[0]['index']), 'rb') as g:
        assert f.read() == g.read()


def test_backend_sweep_direction_equals_the_per_value_api(hip_lib):
    from ctrlhair_amd.ui.backend import Backend
    torch.manual_seed(0)
    be = Backend(2.5, blending=False, weights=_weights(), device=0, max_batch=4)
    be.noise = torch.from_numpy(P.noise_planes(1, 256, NGF, seed=77)).cuda()
    be.set_input_img(((P.synthetic_images(1, 256, seed=3)[0].transpose(1, 2, 0) * 0.5 + 0.5) * 255).astype(np.uint8))
    base_shape, base_mask = be.cur_latent.shape.clone(), be.cur_mask.copy()
    saved = be.copy_latent()

    def same(a, b):                                                          # the bound of tests/test_backend.py for sweep()
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        return d.max() <= 1 and (d > 0).mean() < 1e-3

    values = [-2.5, -1.0, 0.0, 1.0, 2.5]                                      # 5 > max_batch 4
    for att, dim, idx in (('shape', 16, 0), ('texture', 8, 1)):
        d = DS.candidate_direction(dim, [], 4, idx)
        imgs, masks = be.sweep_direction(att, d, values)
        assert len(imgs) == 5 and masks.shape == (5, 256, 256)
        assert torch.equal(be.cur_latent.shape, base_shape) and np.array_equal(be.cur_mask, base_mask)
        for v, img, m in zip(values, imgs, masks):
            be.cur_latent = be.copy_latent(saved)
            be.continue_change_with_direction(att, d.to(be.device), v)
            assert np.array_equal(be.cur_mask, m)
            assert same(be.output(), img)
        be.cur_latent = saved
        be.refresh_cur_mask()
        assert att != 'shape' or len({im.tobytes() for im in imgs}) == 5
    # an index is the special case direction = dirs[idx]
    a, _ = be.sweep('shape', 0, values[:2])
    b, _ = be.sweep_direction('shape', be.shape_dirs[0], values[:2])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        be.sweep_direction('color', d, values)
