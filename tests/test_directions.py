"""Direction search, host side (ctrlhair_amd/directions.py): candidates against the reference's recorded outputs, colour tables, scores
from exact integers, the numpy oracle of the measurements on a case worked out by hand, and the files of the job.  No GPU."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from ctrlhair_amd import directions as DS
from ctrlhair_amd import hostutil as U
from ctrlhair_amd.dataset import shard
from tests import sheet_oracle as SO
from tests.golden import make_direction_golden as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'directions.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('dim', G.DIMS)
@pytest.mark.parametrize('n_existing', G.N_EXISTING)
def test_random_direction_equals_the_reference(golden, dim, n_existing):
    existing = G.existing_dirs(dim, n_existing)
    for s in G.SEEDS:
        d = DS.random_direction(dim, existing, torch.Generator().manual_seed(s))
        assert d.dtype == torch.float32 and tuple(d.shape) == (dim,)
        assert np.array_equal(d.numpy(), golden[f'dir_{dim}_{n_existing}_{s}']), (dim, n_existing, s)     # bit for bit
        d64 = d.numpy().astype(np.float64)
        assert abs(np.linalg.norm(d64) - 1.0) <= 2e-7
        assert all(abs(float(d64 @ e.astype(np.float64))) <= 1e-6 for e in existing)
        assert d[0] >= 0


@pytest.mark.parametrize('draw_type', G.DRAW_TYPES)
def test_colour_tables_equal_the_reference(golden, draw_type):
    lab = G.label_map()
    assert {19, 200, 255} <= set(np.unique(lab).tolist())
    lut = DS.mask_lut(draw_type)
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut[lab], golden[f'mask_rgb_{draw_type}'])
    assert not lut[19:255].any() and (lut[255] == 255).all()


def test_candidates_do_not_depend_on_the_sharding():
    existing = G.existing_dirs(16, 2)
    n = 7
    alone = [DS.candidate_direction(16, existing, 5, i) for i in range(n)]
    assert len({a.numpy().tobytes() for a in alone}) == n
    for world in (1, 2, 3):
        for rank in range(world):
            for i in reversed(shard(list(range(n)), rank, world)):             # another order, other draws in between
                torch.randn(3)
                assert torch.equal(DS.candidate_direction(16, existing, 5, i), alone[i])
    assert not torch.equal(DS.candidate_direction(16, existing, 6, 0), alone[0])
    with pytest.raises(ValueError):
        DS.candidate_direction(16, existing, 5, -1)


def test_stats_oracle_on_a_case_worked_out_by_hand():
    """Two 5 x 7 renders, uint8 images of one colour each: render 0 = (10, 20, 30), render 1 = (13, 18, 30).
    Render 0: hair at (y, x) = (1,2) (1,3) (2,2) (2,3), label 1 elsewhere.  count 4; sum x = 2+3+2+3 = 10; sum y = 1+1+2+2 = 6;
      sum x^2 = 4+9+4+9 = 26; sum y^2 = 1+1+4+4 = 10; box y 1..2, x 2..3; colour sums 4 * (10, 20, 30) = (40, 80, 120); ref = -1, so
      columns 12..15 are 0.
    Render 1: hair at (2,2) (2,3) (3,2) (3,3) (3,4), label 2 at (0,0), label 1 elsewhere.  count 5; sum x = 2+3+2+3+4 = 14;
      sum y = 2+2+3+3+3 = 13; sum x^2 = 4+9+4+9+16 = 42; sum y^2 = 4+4+9+9+9 = 35; box y 2..3, x 2..4; colour sums
      5 * (13, 18, 30) = (65, 90, 150); against render 0: labels differ at (1,2) (1,3) (3,2) (3,3) (3,4) (0,0) = 6; hair in both at
      (2,2) (2,3) = 2; hair in either 4 + 5 - 2 = 7; |d| per pixel = 3 + 2 + 0 = 5, over the union 35."""
    lab = np.ones((2, 5, 7), np.uint8)
    for y, x in ((1, 2), (1, 3), (2, 2), (2, 3)):
        lab[0, y, x] = 13
    for y, x in ((2, 2), (2, 3), (3, 2), (3, 3), (3, 4)):
        lab[1, y, x] = 13
    lab[1, 0, 0] = 2
    img = np.empty((2, 5, 7, 3), np.uint8)
    img[0], img[1] = (10, 20, 30), (13, 18, 30)
    want = np.array([[4, 10, 6, 26, 10, 1, 2, 2, 3, 40, 80, 120, 0, 0, 0, 0],
                     [5, 14, 13, 42, 35, 2, 3, 2, 4, 65, 90, 150, 6, 2, 35, 7]], np.int64)
    assert np.array_equal(SO.sweep_stats(img, 1, lab, [-1, 0]), want)
    # the same colours as floats go through the conversion: (u + 0.25) / 127.5 - 1 truncates back to u
    f = ((img.astype(np.float64) + 0.25) / 127.5 - 1.0).astype(np.float32).transpose(0, 3, 1, 2)
    assert np.array_equal(SO.sweep_stats(f, 0, lab, [-1, 0]), want)
    none = SO.sweep_stats(img[:1], 1, np.zeros((1, 5, 7), np.uint8), [0])
    assert (none[0, 5:9] == -1).all() and none[0, 0] == 0 and not none[0, 9:].any()


def test_unfused_conversion_values():
    """Inputs whose byte differs between x * 127.5 + 127.5 with two roundings and with one (a fused multiply-add)."""
    xs = [float.fromhex(h) for h in ('-0x1.676768p-1', '-0x1.31313ap-4', '-0x1.575758p-1', '-0x1.bfbfc0p-1', '-0x1.c5c5c8p-2',
                                     '-0x1.11111ap-4')]
    assert SO.to_u8(np.array(xs, np.float32)).tolist() == [38, 118, 42, 16, 71, 119]
    fused = [int(np.float32(np.float64(np.float32(x)) * 127.5 + 127.5)) for x in xs]      # exact product and sum, one rounding
    assert fused == [37, 117, 41, 15, 70, 118]
    assert SO.to_u8(np.array([1, -1, 1.5, -1.5, np.nan, np.inf, -np.inf], np.float32)).tolist() == [255, 0, 255, 0, 0, 255, 0]


def _growing_rectangle(V=3, H=8, W=8):
    """Hair over x 2..5, rows 1..1+v for value v: one more row per value."""
    lab = np.ones((V, H, W), np.uint8)
    for v in range(V):
        lab[v, 1:2 + v, 2:6] = 13
    img = np.full((V, H, W, 3), 100, np.uint8)
    return SO.sweep_stats(img, 1, lab, [0] * V)[None]                          # [1,V,16]


def test_score_from_integer_rows():
    st = _growing_rectangle()
    assert st[0, :, 0].tolist() == [4, 8, 12] and st[0, :, 12].tolist() == [0, 4, 8] and st[0, :, 6].tolist() == [1, 2, 3]
    sc = DS.score('shape', st, [-1.0, 0.0, 1.0], 8, 8)
    assert sc['effect'] == 8 / 64 and sc['monotone'] == 1.0                     # exact: 8 changed labels of 64
    assert sc['area'] == pytest.approx(4 / 64, rel=1e-12) and sc['length'] == pytest.approx(1.0, rel=1e-12)
    assert sc['area'] > 0 and sc['length'] > 0 and sc['centroid_y'] == pytest.approx(0.5, rel=1e-12) and abs(sc['centroid_x']) < 1e-12
    # texture: colour change 0, 6, 12 levels summed over 3 channels inside a union of 4 pixels
    tx = np.zeros((2, 3, 16), np.int64)
    tx[0, :, 0], tx[0, :, 15], tx[0, :, 14] = 4, 4, [0, 24, 48]
    tx[0, :, 9], tx[0, :, 10], tx[0, :, 11] = [400, 408, 416], 400, [400, 396, 392]
    sc = DS.score('texture', tx, [-1.0, 0.0, 1.0], 8, 8)                         # image 1: no hair at all, column 15 = 0
    assert sc['effect'] == (48 / 12 + 0.0) / 2 and np.isfinite(sc['effect'])
    assert sc['monotone'] == 1.0 and sc['colour_drift'] == (4.0 + 0.0) / 2
    falling = tx.copy()
    falling[0, :, 14] = [0, 48, 24]
    assert DS.score('texture', falling, [-1.0, 0.0, 1.0], 8, 8)['monotone'] == 0.75
    with pytest.raises(ValueError):
        DS.score('colour', tx, [-1.0, 0.0, 1.0], 8, 8)


def test_direction_files_load_through_checkpoints(tmp_path):
    from ctrlhair_amd.checkpoints import _load_dirs
    from ctrlhair_amd.hair_editor import HairEditor
    used = tmp_path / 'texture_dir_used'
    out = tmp_path / 'find'
    (out / 'texture_dir_1').mkdir(parents=True)
    cands = [DS.candidate_direction(8, [], 0, i) for i in range(3)]
    for i, d in enumerate(cands):
        DS.write_direction(str(out / 'texture_dir_1' / f'{i}.pkl'), d)
    with open(out / 'texture_dir_1' / '2.pkl', 'rb') as f:
        back = pickle.load(f)
    assert isinstance(back, torch.Tensor) and back.dtype == torch.float32 and torch.equal(back, cands[2])
    assert DS.load_used(str(used)) == []
    first = DS.use_direction(str(out), 'texture', 2, str(used))
    assert os.path.basename(first) == '00.pkl'
    (out / 'texture_dir_2').mkdir()
    DS.write_direction(str(out / 'texture_dir_2' / '0.pkl'), DS.candidate_direction(8, DS.load_used(str(used)), 0, 0))
    assert os.path.basename(DS.use_direction(str(out), 'texture', 0, str(used))) == '01.pkl'
    with pytest.raises(FileNotFoundError):
        DS.use_direction(str(out), 'texture', 5, str(used))
    loaded = _load_dirs(str(used))
    assert len(loaded) == 2 and np.array_equal(loaded[0], cands[2].numpy()) and loaded[1].dtype == np.float32
    assert abs(float(loaded[0] @ loaded[1])) <= 1e-6
    shape_dirs = [DS.candidate_direction(16, [], 1, i).numpy() for i in range(2)]
    cpu = torch.device('cpu')
    stub = types.SimpleNamespace(sean_model=None, device=cpu, face_parsing=None, mask_generator=None,
                                 solver_feature=types.SimpleNamespace(dis=None, gen=None, rgb_model=None))
    he = HairEditor(True, True, models=stub, texture_dirs=loaded, shape_dirs=shape_dirs, cap_threads=False)
    assert len(he.texture_dirs) == 2 and torch.equal(he.texture_dirs[0], cands[2]) and tuple(he.shape_dirs[1].shape) == (16,)


def test_merge_scores_and_sheet_option(tmp_path):
    import json
    for r, recs in enumerate(([{'index': 0, 'effect': 0.1}, {'index': 2, 'effect': 0.5}], [{'index': 1, 'effect': 0.5}])):
        with open(tmp_path / ('scores.rank%03dof002.json' % r), 'w') as f:
            json.dump(recs, f)
    with open(tmp_path / 'scores.rank002of003.json', 'w') as f:                # left by an earlier run on three ranks: not read
        json.dump([{'index': 2, 'effect': 9.0}], f)
    merged = DS.merge_scores(str(tmp_path), world=2)
    assert [m['index'] for m in merged] == [1, 2, 0]
    with open(tmp_path / 'scores.json') as f:
        assert json.load(f) == merged
    with pytest.raises(FileNotFoundError):
        DS.merge_scores(str(tmp_path), world=4)
    assert DS.parse_sheets('all') == ('all', 0) and DS.parse_sheets('top:20') == ('top', 20) and DS.parse_sheets('none') == ('none', 0)
    for bad in ('top', 'top:0', 'some'):
        with pytest.raises(ValueError):
            DS.parse_sheets(bad)


def test_search_images_and_use_direction_commands(tmp_path, capsys):
    """The parts of the job's command line that need no GPU: which images are read and how, and the use-direction command."""
    from PIL import Image
    from ctrlhair_amd import dataset as D
    rng = np.random.default_rng(0)
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    pics = {}
    for name, (h, w) in (('b.png', (16, 16)), ('a.png', (24, 20)), ('c.png', (16, 16))):
        pics[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(pics[name]).save(img_dir / name)
    (img_dir / 'notes.txt').write_text('not an image')
    x = D.load_search_images(str(img_dir), 16, 2)                                # the first two of the sorted names
    assert x.shape == (2, 3, 16, 16) and x.dtype == np.float32 and x.min() >= -1 and x.max() <= 1
    want_b = (pics['b.png'].transpose(2, 0, 1) / 127.5 - 1.0).astype(np.float32)
    assert np.array_equal(x[1], want_b)                                          # already 16 x 16: only rescaled
    want_a = U.resize_bilinear(pics['a.png'], (16, 16))                          # 24 x 20 -> cv2-bilinear 16 x 16
    assert np.array_equal(x[0], (want_a.transpose(2, 0, 1) / 127.5 - 1.0).astype(np.float32))
    lst = tmp_path / 'names.txt'
    lst.write_text('# chosen by hand\nc.png\n\nb.png\n')
    y = D.load_search_images(str(img_dir), 16, 10, str(lst))                     # the list's order, comments and blanks skipped
    assert y.shape[0] == 2 and np.array_equal(y[1], want_b) and not np.array_equal(y[0], want_b)
    with pytest.raises(ValueError):
        D.load_search_images(str(img_dir), 16, 0)
    out, used = tmp_path / 'find', tmp_path / 'shape_dir_used'
    (out / 'shape_dir_1').mkdir(parents=True)
    d = DS.candidate_direction(16, [], 3, 7)
    DS.write_direction(str(out / 'shape_dir_1' / '7.pkl'), d)
    D.main(['use-direction', str(out), 'shape', '7', str(used)])
    assert capsys.readouterr().out.strip() == str(used / '00.pkl')
    assert np.array_equal(DS.load_used(str(used))[0], d.numpy())
