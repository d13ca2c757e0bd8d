"""The CPU side of the PNG encoder's caller-given match distances: the test tools themselves (tests/deflate_tokens.py decodes what zlib
writes, tests/png_dist_oracle.py replays what it parses), the parse rule's invariants, and the host-side argument checks."""
import zlib

import numpy as np
import pytest

from ctrlhair_amd import directions as DS
from ctrlhair_amd import pngenc as PE
from tests import deflate_tokens as DT
from tests import png_dist_oracle as DO
from tests import png_oracle as PO

K = 32768
LISTS = [(), (132,), (3, 132), (128, 129), (32767,)]


def _inputs():
    rng = np.random.default_rng(11)
    sheet = DO.sheet(2, 3, 40, 4)                                                          # column pitch (40 + 4) * 3 = 132
    return {'sheet': PO.filtered_stream(sheet)[0][:K], 'sheet0': PO.filtered_stream(sheet, 0)[0][K:],
            'tile': DO.tile(5000).tobytes(), 'noise': rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), 'zeros': bytes(2000),
            'long': np.tile(rng.integers(0, 256, 32767, dtype=np.uint8), 2)[:K].tobytes()}


INPUTS = _inputs()


@pytest.mark.parametrize('how', ['level1', 'level6', 'rle', 'fixed', 'level0'])
def test_tokenizer_decodes_what_zlib_writes(how):
    level, strategy = {'level1': (1, zlib.Z_DEFAULT_STRATEGY), 'level6': (6, zlib.Z_DEFAULT_STRATEGY), 'rle': (6, zlib.Z_RLE),
                       'fixed': (6, zlib.Z_FIXED), 'level0': (0, zlib.Z_DEFAULT_STRATEGY)}[how]
    for name in ('sheet', 'tile', 'noise', 'zeros'):
        data = INPUTS[name]
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        stream = co.compress(data[:len(data) // 2]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[len(data) // 2:]) + co.flush()
        tokens, out, blocks = DT.inflate_zlib(stream)
        assert out == zlib.decompress(stream) == data, (how, name)
        assert DO.replay(tokens) == b''.join(out[b.out_start:b.out_end] for b in blocks if b.btype != 0)
        assert blocks[-1].final and not any(b.final for b in blocks[:-1])
        assert [b.out_start for b in blocks[1:]] == [b.out_end for b in blocks[:-1]] and blocks[-1].out_end == len(data)
        kinds = {b.btype for b in blocks}
        if how == 'level0':
            assert kinds == {0} and not tokens
        if how == 'fixed':
            assert 2 not in kinds and (1 in kinds or name == 'noise')                      # (zlib stores what a fixed code would enlarge)
        if how == 'rle':
            assert all(t[2] == 1 for t in tokens if t[0] == 'M')
        if how in ('level1', 'level6') and name == 'tile':
            assert any(t[0] == 'M' and t[2] == 120 for t in tokens)
    with pytest.raises(ValueError):
        DT.inflate_zlib(zlib.compress(b'abc' * 50)[:-1])
    with pytest.raises(ValueError):
        DT.inflate_zlib(zlib.compress(b'abc' * 50) + b'\0')


@pytest.mark.parametrize('D', LISTS)
@pytest.mark.parametrize('name', sorted(INPUTS))
def test_parse_replays_and_stays_inside_the_chunk(name, D):
    x = INPUTS[name]
    tokens = DO.parse(x, D)
    assert DO.replay(tokens) == x
    pos = 0
    for t in tokens:
        if t[0] == 'M':
            assert t[2] in (1,) + D and 3 <= t[1] <= 258 and pos - t[2] >= 0, (t, pos)
            pos += t[1]
        else:
            pos += 1
    assert pos == len(x)
    matches = [t for t in tokens if t[0] == 'M']
    if name == 'noise':
        assert len(matches) < 5
    if name == 'zeros':
        assert {t[2] for t in matches} == {1} and tokens[0] == ('L', 0)
    if name == 'tile' and 120 in D:
        assert any(t[2] == 120 for t in matches)
    if name == 'long' and D == (32767,):                                                   # one interval [32767, 32768): a single position, a literal
        assert not any(t[2] == 32767 for t in matches)


def test_parse_prefers_the_stride_on_a_sheet():
    x = INPUTS['sheet']
    with_stride = [t for t in DO.parse(x, (132,)) if t[0] == 'M' and t[2] == 132]
    assert sum(t[1] for t in with_stride) > len(x) // 3                                    # most bytes outside the ellipses repeat the column before
    assert len(DO.parse(x, (132,))) < len(DO.parse(x, ())) * 3 // 4


def test_parse_without_distances_is_the_run_rule():
    """DESIGN.md section 16, *Runs*: a run of L equal bytes is the literal, (L - 1) // 258 matches of 258 and the remainder (L - 1) % 258
    as one match if it is >= 3, else as literals."""
    for L in (1, 2, 3, 4, 257, 258, 259, 260, 516, 517, 518):
        x = bytes([9]) + bytes([5]) * L + bytes([7])
        full, rem = divmod(L - 1, 258)
        want = [('L', 9), ('L', 5)] + [('M', 258, 1)] * full + ([('M', rem, 1)] if rem >= 3 else [('L', 5)] * rem) + [('L', 7)]
        assert DO.parse(x, ()) == want, L
        assert DO.parse(x, (2,))[:2] == want[:2]


def test_parse_ties_go_to_the_earlier_distance():
    rng = np.random.default_rng(5)
    x = (rng.permutation(200) % 200).astype(np.uint8)                                      # 200 distinct bytes: no interval of any distance
    d, q = 50, 120
    x[q - 1:q + 10] = 33                                                                   # eq_1 holds on [q, q + 9]
    x[q - 5 - d:q + 5 - d] = x[q - 5:q + 5]                                                # eq_d holds on [q - 5, q + 4], 10 long as well
    c = DO.classes(x.tobytes(), (d,))
    assert list(c[q - 5:q]) == [1] * 5 and list(c[q:q + 10]) == [0] * 10
    tokens = DO.parse(x.tobytes(), (d,))
    k = tokens.index(('M', 5, d))
    assert tokens[k + 1] == ('M', 10, 1)
    assert DO.replay(tokens) == x.tobytes()


def test_zlib_chunked_is_the_sum_over_chunks():
    s = INPUTS['sheet'] + INPUTS['noise']
    assert DO.zlib_chunked(s, K, 6) == 8 + (DO.zlib_chunked(s[:K], K, 6) - 8) + (5 + 3000)
    assert DO.zlib_chunked(INPUTS['sheet'], K, 6) < DO.zlib_chunked(INPUTS['sheet'], K, 1) < PO.rle_yardstick(INPUTS['sheet'], K)


def test_sheet_shapes():
    assert DO.sheet(2, 3, 40, 0).shape == (80, 160, 3) and len(PO.filtered_stream(DO.sheet(2, 3, 40, 0))[0]) == 38480
    s = DO.sheet(2, 3, 40, 4)
    assert s.shape == (80, 172, 3) and len(PO.filtered_stream(s)[0]) == 41360
    assert (s[:, 40:44] == 255).all() and not np.array_equal(s[:40, :40], s[:40, 44:84])
    outside = s[:40, :40] == s[:40, 44:84]
    assert 0.4 < outside.mean() < 0.9                                                      # the columns agree outside the ellipse only


def test_contact_sheet_distances():
    assert DS.sheet_png_distances(6, 256, 0) == (768,)
    assert DS.sheet_png_distances(4, 40, 4) == (132,)
    assert DS.sheet_png_distances(1, 256, 0) == ()
    assert DS.sheet_png_distances(3, 10922, 0) == (32766,) and DS.sheet_png_distances(3, 10923, 0) == ()


def test_distances_are_checked_on_the_host():
    assert PE.check_distances(()) == () and PE.check_distances([768]) == (768,) and PE.check_distances((2, 32767, np.int64(9))) == (2, 32767, 9)
    for bad in ((1,), (0,), (32768,), (-3,), (5, 5), (2, 3, 2), (2, 3, 4, 5), (2.0,), ('7',), (True,), 7, None):
        with pytest.raises(ValueError):
            PE.check_distances(bad)


def test_cli_parses_png_stride(monkeypatch, tmp_path):
    """`directions --png device --png-stride` reaches find_directions as png_stride=True; the default is off; host + stride is refused."""
    import torch
    from ctrlhair_amd import dataset as D, pipeline
    seen = []
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_: None)
    monkeypatch.setattr(pipeline, 'EditPipeline', lambda *a, **k: 'pipe')
    monkeypatch.setattr(DS, 'DirectionSearch', lambda *a, **k: 'search')
    monkeypatch.setattr(DS, 'merge_scores', lambda *a, **k: [])
    monkeypatch.setattr(D, 'load_search_images', lambda *a, **k: np.zeros((1, 3, 8, 8), np.float32))
    monkeypatch.setattr(DS, 'find_directions', lambda *a, **k: seen.append((k.get('png'), k.get('png_stride'))) or [])
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.chdir(tmp_path)
    cli = ['directions', 'imgs', '--att', 'shape']
    D.main(cli)
    D.main(cli + ['--png', 'device'])
    D.main(cli + ['--png', 'device', '--png-stride'])
    assert seen == [('host', False), ('device', False), ('device', True)]
    for bad in (['--png-stride'], ['--png', 'host', '--png-stride']):
        with pytest.raises(SystemExit):
            D.main(cli + bad)
    assert len(seen) == 3


def test_find_directions_hands_the_sheets_distances_to_the_encoder(monkeypatch, tmp_path):
    import types
    calls = []

    class Enc:
        def __init__(self, handle, device):
            pass

        def write(self, paths, images, **kw):
            calls.append(kw)

    class Search:
        handle, device, S = 'handle', 'cpu', 8

        def sweep(self, att, d, values):
            return 'images', 'masks'

        def stats(self, images, masks):
            return 'stats'

        def sheet(self, att, images, masks, cell=None):
            return types.SimpleNamespace(canvas=np.zeros((1, 1, 3), np.uint8), png_distances=lambda: (768,))

    monkeypatch.setattr(PE, 'PngEncoder', Enc)
    monkeypatch.setattr(DS, 'score', lambda *a, **k: {'effect': 0.0})
    kw = dict(n=1, values=[0.0])
    DS.find_directions(Search(), 'texture', [], str(tmp_path / 'a'), png='device', **kw)
    DS.find_directions(Search(), 'texture', [], str(tmp_path / 'b'), png='device', png_stride=True, **kw)
    assert calls == [{}, {'distances': (768,)}]                                            # without the option the call is the one of before
    with pytest.raises(ValueError):
        DS.find_directions(Search(), 'texture', [], str(tmp_path / 'c'), png='host', png_stride=True, **kw)
    assert len(calls) == 2
