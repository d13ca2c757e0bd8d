"""CPU-only: the host side of the median style codes (ctrlhair_amd/stylestats.py) and the oracles of tests/medoid_oracle.py.

The float64 difference-form oracle must reproduce the rows the reference's own get_mean_code.py chose for the golden input
(tests/golden/medoid_golden.npz, recorded by tests/golden/make_medoid_golden.py), and the restated reference arithmetic must show the
failure on saturated codes that motivates the difference form."""
import os

import numpy as np
import pytest

from ctrlhair_amd import stylestats as SS
from tests import medoid_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'medoid_golden.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_f64_oracle_reproduces_reference_rows(golden):
    codes = O.golden_codes()
    assert np.array_equal(SS.presence(codes), golden['presence'])
    index, count, _, gaps = O.median_rows_f64(codes)
    assert np.array_equal(count, golden['presence'].sum(axis=0))
    assert count[O.GOLDEN_ONE] == 1 and count[O.GOLDEN_NONE] == 0
    assert np.array_equal(golden['written'], count > 0)
    assert np.array_equal(index, golden['index'])
    for j in range(O.N_REGIONS):
        if count[j]:
            assert np.array_equal(codes[index[j], j], golden['rows'][j])
        if count[j] > 1:
            assert gaps[j] > 1e-3, (j, gaps[j])             # the reference's float32 slop (~5e-6) cannot decide any of them


def test_reference_arithmetic_restated(golden):
    """The float32 Gram restatement is the reference: it picks the recorded rows too."""
    codes = O.golden_codes()
    for j in range(O.N_REGIONS):
        rows = np.nonzero(golden['presence'][:, j])[0]
        if len(rows):
            m, _ = O.reference_f32(codes[rows, j])
            assert rows[m] == golden['index'][j]


def test_gram_identity_fails_on_saturated_codes():
    """130 codes of 0.79 + 1e-3 N(0,1): the reference's float32 row sums are wrong by percents and it picks another code; a float32
    difference-form evaluation stays within 1e-6 and picks the float64 medoid."""
    x = O.saturated()
    m, s, gap = O.medoid_f64(x)
    assert gap > 1e-3, gap
    rm, rs = O.reference_f32(x)
    err = np.abs(rs.astype(np.float64) - s).max() / s.min()
    assert rm != m and err > 1e-2, (rm, m, err)
    d = x[:, None, :] - x[None, :, :]                                        # float32 throughout
    s32 = np.sqrt((d * d).sum(axis=2, dtype=np.float32)).astype(np.float64).sum(axis=1)
    assert np.abs(s32 - s).max() / s.min() < 1e-6 and int(np.argmin(s32)) == m


def test_presence_and_compaction():
    codes = O.golden_codes()
    pres = O.golden_presence()
    rows, off, source = SS.compact(codes)
    assert off.dtype == np.int64 and off[0] == 0 and np.array_equal(np.diff(off), pres.sum(axis=0))
    assert rows.dtype == np.float32 and rows.shape == (pres.sum(), O.STYLE_LEN) and rows.flags.c_contiguous
    for j in range(O.N_REGIONS):
        src = source[off[j]:off[j + 1]]
        assert np.array_equal(src, np.nonzero(pres[:, j])[0])                # input order kept
        assert np.array_equal(rows[off[j]:off[j + 1]], codes[src, j])
    # a row with a single non-zero value counts, an all-zero row does not
    codes[:] = 0
    codes[2, 4, 17] = 1e-30
    assert SS.presence(codes).sum() == 1 and SS.presence(codes)[2, 4]


def test_as_code_array_accepts_dict_and_tensor():
    import torch
    codes = O.golden_codes()[:5]
    d = {f'ds___{i:03d}': codes[i] for i in range(5)}
    a, keys = SS.as_code_array(d)
    assert keys == list(d) and np.array_equal(a, codes)
    a, keys = SS.as_code_array(torch.from_numpy(codes))
    assert keys is None and np.array_equal(a, codes)
    with pytest.raises(ValueError):
        SS.as_code_array(codes[:, :18])


def test_finish_maps_indices_and_keeps_packaged_rows():
    codes = O.golden_codes()
    rows, off, source = SS.compact(codes)
    index64, count, mean64, _ = O.median_rows_f64(codes)
    local = np.array([0 if count[j] == 0 else int(np.nonzero(source[off[j]:off[j + 1]] == index64[j])[0][0]) for j in range(19)])
    local[O.GOLDEN_NONE] = -1
    mean = np.nan_to_num(mean64).astype(np.float32)
    res = SS.finish(codes, off, source, local, mean, keys=None)
    assert np.array_equal(res['index'], index64) and np.array_equal(res['count'], count)
    packaged = SS.load_mean_style_code()
    for j in range(19):
        if count[j]:
            assert np.array_equal(res['median'][j], codes[index64[j], j]) and np.array_equal(res['mean'][j], mean[j])
        else:
            assert res['index'][j] == -1
            assert np.array_equal(res['median'][j], packaged['median'][j]) and np.array_equal(res['mean'][j], packaged['mean'][j])


def test_npz_and_tree_round_trip(tmp_path):
    packaged = SS.load_mean_style_code()
    res = {'median': packaged['median'][::-1].copy(), 'mean': packaged['mean'] * np.float32(0.5)}
    path = str(tmp_path / 'mean_style_code.npz')
    SS.save_mean_style_code(path, res)
    with np.load(path) as z, np.load(SS.PACKAGED) as p:
        assert sorted(z.files) == sorted(p.files)
        for k in p.files:
            assert z[k].dtype == p[k].dtype and z[k].shape == p[k].shape
    back = SS.load_mean_style_code(path)
    assert np.array_equal(back['median'], res['median']) and np.array_equal(back['mean'], res['mean'])
    SS.write_reference_tree(str(tmp_path / 'styles_test'), res)
    one = np.load(str(tmp_path / 'styles_test' / 'mean_style_code' / 'median' / '7' / 'ACE.npy'))
    assert one.dtype == np.float32 and one.shape == (512,) and np.array_equal(one, res['median'][7])
    tree = SS.read_reference_tree(str(tmp_path / 'styles_test'))
    assert np.array_equal(tree['median'], res['median']) and np.array_equal(tree['mean'], res['mean'])


@pytest.mark.parametrize('bad', ['keys', 'shape', 'dtype'])
def test_malformed_file_is_rejected(tmp_path, bad):
    p = SS.load_mean_style_code()
    arrs = {'keys': {'median': p['median']}, 'shape': {'median': p['median'][:18], 'mean': p['mean']},
            'dtype': {'median': p['median'].astype(np.float64), 'mean': p['mean']}}[bad]
    path = str(tmp_path / 'bad.npz')
    np.savez(path, **arrs)
    with pytest.raises(ValueError):
        SS.load_mean_style_code(path)
    with pytest.raises(ValueError):
        SS.save_mean_style_code(str(tmp_path / 'x.npz'), {'median': p['median'][:3], 'mean': p['mean']})


def test_editor_rejects_malformed_file_before_building_models(tmp_path):
    from ctrlhair_amd.hair_editor import HairEditor
    path = str(tmp_path / 'bad.npz')
    np.savez(path, median=np.zeros((19, 512), np.float32))
    with pytest.raises(ValueError):
        HairEditor(weights='procedural', mean_style_code=path, cap_threads=False)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert SS.StyleMedoid().median_style_codes(O.golden_codes())['count'][O.GOLDEN_NONE] == 0
    else:
        with pytest.raises(RuntimeError):
            SS.StyleMedoid()
