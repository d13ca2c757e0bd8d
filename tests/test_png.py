"""CPU-only: the host half of the PNG encoder (ctrlhair_amd/pngenc.py) -- the container around a zlib stream and the Adler-32
combination the gather kernel restates --, the numpy oracle of the row filters (tests/png_oracle.py), and the `png=` option of the jobs
and their command lines."""
import io
import types
import zlib

import numpy as np
import pytest

from ctrlhair_amd import pngenc as PE
from tests import png_oracle as PO

MODES = {1: 'L', 3: 'RGB', 4: 'RGBA'}


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 31), (70, 53)])
def test_wrap_png_decodes_to_the_pixels(shape, C):
    from PIL import Image
    H, W = shape
    img = np.random.default_rng(H * 100 + C).integers(0, 256, (H, W, C), dtype=np.uint8)
    for filt in (-1, 0, 1, 2, 3, 4):
        stream, types_ = PO.filtered_stream(img, filt)
        assert len(stream) == H * (1 + W * C) and (filt < 0 or (types_ == filt).all())
        png = PE.wrap_png(zlib.compress(stream), H, W, C)
        im = Image.open(io.BytesIO(png))
        im.load()
        assert im.mode == MODES[C] and im.size == (W, H)
        assert np.array_equal(np.asarray(im).reshape(H, W, C), img), filt


def test_wrap_png_splits_long_streams_and_checks_arguments(monkeypatch):
    from PIL import Image
    img = np.random.default_rng(0).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    z = zlib.compress(PO.filtered_stream(img)[0], 0)
    monkeypatch.setattr(PE, 'IDAT_MAX', 1000)
    png = PE.wrap_png(z, 40, 50, 3)
    assert png.count(b'IDAT') == (len(z) + 999) // 1000 >= 6
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), img)
    for bad in ((40, 50, 2), (0, 50, 3), (40, 0, 3)):
        with pytest.raises(ValueError):
            PE.wrap_png(z, *bad)


def test_filter_oracle_on_a_hand_computed_case():
    # rows (10,20,30)(13,26,39)(250,5,100) and (12,22,29)(20,20,20)(0,255,7); a = one pixel left, b = above, c = above left
    img = np.array([[[10, 20, 30], [13, 26, 39], [250, 5, 100]], [[12, 22, 29], [20, 20, 20], [0, 255, 7]]], np.uint8)
    rows = PO.filter_rows(img)
    assert rows[0].tolist() == [[10, 20, 30, 13, 26, 39, 250, 5, 100], [12, 22, 29, 20, 20, 20, 0, 255, 7]]
    assert rows[1].tolist() == [[10, 20, 30, 3, 6, 9, 237, 235, 61], [12, 22, 29, 8, 254, 247, 236, 235, 243]]                 # x - a
    assert rows[2].tolist() == [[10, 20, 30, 13, 26, 39, 250, 5, 100], [2, 2, 255, 7, 250, 237, 6, 250, 163]]                  # x - b
    # x - floor((a + b) / 2); row 1: (0+10)/2, (0+20)/2, (0+30)/2, (12+13)/2, (22+26)/2, (29+39)/2, (20+250)/2, (20+5)/2, (20+100)/2
    assert rows[3].tolist() == [[10, 20, 30, 8, 16, 24, 244, 248, 81], [7, 12, 14, 8, 252, 242, 121, 243, 203]]
    # Paeth: row 0 predicts a (b = c = 0); row 1, first pixel predicts b (a = c = 0); then p = a + b - c:
    #   (12,13,10) p 15 -> b 13; (22,26,20) p 28 -> b 26; (29,39,30) p 38 -> b 39; (20,250,13) p 257 -> b 250; (20,5,26) p -1 -> b 5;
    #   (20,100,39) p 81 -> b 100
    assert rows[4].tolist() == [[10, 20, 30, 3, 6, 9, 237, 235, 61], [2, 2, 255, 7, 250, 237, 6, 250, 163]]
    stream, types_ = PO.filtered_stream(img, -1)
    # sums of |int8|: row 0: none 10+20+30+13+26+39+6+5+100 = 249, sub 10+20+30+3+6+9+19+21+61 = 179, up = none, avg 10+20+30+8+16+24+12+8+81 =
    # 209, paeth = sub -> 1 (the lower of the tied 1 and 4); row 1: none 12+22+29+20+20+20+0+1+7 = 131, sub 12+22+29+8+2+9+20+21+13 = 136,
    # up = paeth 2+2+1+7+6+19+6+6+93 = 142, avg 7+12+14+8+4+14+121+13+53 = 246 -> 0
    assert types_.tolist() == [1, 0]
    assert list(stream) == [1] + rows[1][0].tolist() + [0] + rows[0][1].tolist()
    for filt in (-1, 0, 1, 2, 3, 4):
        assert np.array_equal(PO.unfilter(PO.filtered_stream(img, filt)[0], 2, 3, 3), img)
    grey = np.random.default_rng(3).integers(0, 256, (6, 7), dtype=np.uint8)
    assert np.array_equal(PO.unfilter(PO.filtered_stream(grey)[0], 6, 7, 1)[:, :, 0], grey)                                    # [H,W] is C = 1


def test_yardsticks_are_valid_deflate_sizes():
    zeros = bytes(32768)
    assert PO.rle_yardstick(zeros, 32768) < 100 < PO.huffman_only(zeros)
    noise = np.random.default_rng(0).integers(0, 256, 40000, dtype=np.uint8).tobytes()
    assert PO.rle_yardstick(noise, 32768) == 8 + 40000 + 2 * 5                                                                  # stored, both chunks


def test_adler32_combine_equals_zlib():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()
    for cut in [0, 1, 5552, 65520, 65521, 100000, len(data) - 1, len(data)] + [int(v) for v in rng.integers(0, len(data), 8)]:
        x, y = data[:cut], data[cut:]
        assert PE.adler32_combine(zlib.adler32(x), zlib.adler32(y), len(y)) == zlib.adler32(data), cut
    ff = b'\xff' * 70000                                                                                                        # sums that wrap
    assert PE.adler32_combine(zlib.adler32(ff[:33333]), zlib.adler32(ff[33333:]), 70000 - 33333) == zlib.adler32(ff)
    # chunk by chunk, as the device does it, with a zero-length part in the middle
    parts = [data[:32768], data[32768:65536], b'', data[65536:]]
    a = zlib.adler32(b'')
    for p in parts:
        a = PE.adler32_combine(a, zlib.adler32(p), len(p))
    assert a == zlib.adler32(data)


# ---- the option ----------------------------------------------------------------------------------------------------------------------
def test_bogus_png_mode_raises_before_any_work(tmp_path):
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import directions as DS
    (tmp_path / 'in').mkdir()
    with pytest.raises(ValueError, match='png'):
        DS.find_directions(None, 'shape', [], str(tmp_path / 'o'), n=1, png='bogus')
    stub = types.SimpleNamespace(face_parsing=types.SimpleNamespace(handle=None, device=None), handle=None, device=None)
    with pytest.raises(ValueError, match='png'):
        D.extract_masks(stub, str(tmp_path / 'in'), str(tmp_path / 'l'), png='bogus')
    with pytest.raises(ValueError, match='png'):
        D.crop_faces(stub, str(tmp_path / 'in'), str(tmp_path / 'c'), 'ds', {}, png='bogus')
    with pytest.raises(ValueError, match='png'):
        D.uncrop_faces(stub, str(tmp_path / 'in'), str(tmp_path / 'in'), str(tmp_path / 'u'), 'ds', {}, png='bogus')
    assert PE.check_png_mode('host') == 'host' and PE.check_png_mode('device') == 'device'


class _FakeSearch:
    """What find_directions touches of a DirectionSearch, without a GPU."""
    S, handle, device = 8, None, None

    def sweep(self, att, d, values):
        return np.zeros((1, len(values), 3, 8, 8), np.float32), np.zeros((1, len(values), 256, 256), np.uint8)

    def stats(self, images, masks):
        return np.zeros((1, images.shape[1], 16), np.int64)

    def sheet(self, att, images, masks, cell=None):
        return types.SimpleNamespace(numpy=lambda: np.full((16, 8, 3), 9, np.uint8), canvas=None)


def test_host_mode_still_goes_through_write_png(tmp_path, monkeypatch):
    from ctrlhair_amd import directions as DS
    seen = []
    monkeypatch.setattr(DS, 'write_png', lambda path, rgb: seen.append((path, rgb.copy())))
    monkeypatch.setattr(PE, 'PngEncoder', lambda *a, **k: pytest.fail('png=host must not build a device encoder'))
    for kw in ({}, {'png': 'host'}):
        seen.clear()
        DS.find_directions(_FakeSearch(), 'shape', [], str(tmp_path / 'o'), n=2, values=[-1.0, 1.0], **kw)
        assert [p.replace(str(tmp_path), '') for p, _ in seen] == ['/o/shape_1/0.png', '/o/shape_1/1.png']
        assert all((rgb == 9).all() and rgb.shape == (16, 8, 3) for _, rgb in seen)


def test_device_mode_hands_the_canvas_to_the_encoder(tmp_path, monkeypatch):
    from ctrlhair_amd import directions as DS
    calls = []

    class Enc:
        def __init__(self, handle, device):
            calls.append('init')

        def write(self, paths, images):
            calls.append((list(paths), images))

    class Canvas:
        def __getitem__(self, k):
            assert k is None
            return 'canvas[None]'

    class Search(_FakeSearch):
        def sheet(self, att, images, masks, cell=None):
            return types.SimpleNamespace(numpy=lambda: pytest.fail('png=device must not download the sheet'), canvas=Canvas())

    monkeypatch.setattr(PE, 'PngEncoder', Enc)
    monkeypatch.setattr(DS, 'write_png', lambda *a: pytest.fail('png=device must not call write_png'))
    DS.find_directions(Search(), 'texture', [], str(tmp_path / 'o'), n=1, values=[0.0], png='device')
    assert calls == ['init', ([str(tmp_path / 'o' / 'texture_1' / '0.png')], 'canvas[None]')]


def _patch_cli(monkeypatch, seen):
    """Replace what the command lines would start on a GPU by recorders."""
    import torch
    from ctrlhair_amd import alignment, dataset as D, directions as DS, hair_editor, lib, pipeline
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_: None)
    monkeypatch.setattr(lib, 'Handle', lambda *a, **k: 'handle')
    monkeypatch.setattr(alignment, 'FaceAligner', lambda *a, **k: 'aligner')
    monkeypatch.setattr(hair_editor, 'HairEditor', lambda *a, **k: 'editor')
    monkeypatch.setattr(pipeline, 'EditPipeline', lambda *a, **k: 'pipe')
    monkeypatch.setattr(DS, 'DirectionSearch', lambda *a, **k: 'search')
    monkeypatch.setattr(DS, 'merge_scores', lambda *a, **k: [])
    monkeypatch.setattr(D, 'load_search_images', lambda *a, **k: np.zeros((1, 3, 8, 8), np.float32))
    monkeypatch.setattr(D, 'load_landmarks', lambda *a, **k: {})
    monkeypatch.setattr(D, 'extract_masks', lambda *a, **k: seen.append(('masks', k.get('png'))) or [])
    monkeypatch.setattr(D, 'crop_faces', lambda *a, **k: seen.append(('crop', k.get('png'))) or ([], []))
    monkeypatch.setattr(D, 'uncrop_faces', lambda *a, **k: seen.append(('uncrop', k.get('png'))) or ([], []))
    monkeypatch.setattr(DS, 'find_directions', lambda *a, **k: seen.append(('directions', k.get('png'))) or [])
    return D


CLI = {'masks': ['masks', 'root', 'ds', '--weights', 'procedural'],
       'crop': ['crop', 'src', 'root', 'ds', '--landmarks', 'lm.npz'],
       'uncrop': ['uncrop', 'photos', 'edits', 'out', '--landmarks', 'lm.npz'],
       'directions': ['directions', 'imgs', '--att', 'shape']}


@pytest.mark.parametrize('job', sorted(CLI))
def test_cli_parses_png(job, monkeypatch, tmp_path):
    seen = []
    D = _patch_cli(monkeypatch, seen)
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.chdir(tmp_path)
    D.main(CLI[job])
    D.main(CLI[job] + ['--png', 'device'])
    D.main(CLI[job] + ['--png', 'host'])
    assert seen == [(job, 'host'), (job, 'device'), (job, 'host')]
    with pytest.raises(SystemExit):
        D.main(CLI[job] + ['--png', 'bogus'])
    assert len(seen) == 3
