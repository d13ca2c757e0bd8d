"""CPU checks of the matte paste-back's oracle (tests/matte_oracle.py) and host arithmetic (alignment.matte_params): the oracle against
a brute-force triple loop, the guided filter's textbook properties, the int32 bound of the integer moments, and the reason those
moments are integers -- float32 window means move the matte by more than half a grey level on the worst case."""
import numpy as np
import pytest

from ctrlhair_amd import alignment as AL
from tests import align_oracle as AO
from tests import matte_cases as MC
from tests import matte_oracle as MO


def _brute(I8, p8, r, eps):
    """Steps 2-4 pixel by pixel and window pixel by window pixel, Python integers and float64."""
    H, W = p8.shape
    a, b = np.zeros((H, W, 3)), np.zeros((H, W))
    for Y in range(H):
        for X in range(W):
            n, sp, sI, sIp, sII = 0, 0, [0, 0, 0], [0, 0, 0], [[0] * 3 for _ in range(3)]
            for v in range(max(Y - r, 0), min(Y + r, H - 1) + 1):
                for u in range(max(X - r, 0), min(X + r, W - 1) + 1):
                    I, p = [int(t) for t in I8[v, u]], int(p8[v, u])
                    n, sp = n + 1, sp + p
                    for c in range(3):
                        sI[c] += I[c]
                        sIp[c] += I[c] * p
                        for d in range(3):
                            sII[c][d] += I[c] * I[d]
            den = float(n) ** 2 * 65025.0
            cov = np.array([[float(n * sII[c][d] - sI[c] * sI[d]) / den for d in range(3)] for c in range(3)])
            cIp = np.array([float(n * sIp[c] - sI[c] * sp) / den for c in range(3)])
            a[Y, X] = np.linalg.solve(cov + eps * np.eye(3), cIp)
            b[Y, X] = sp / (255.0 * n) - sum(a[Y, X, c] * (sI[c] / (255.0 * n)) for c in range(3))
    a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    q = np.zeros((H, W))
    for Y in range(H):
        for X in range(W):
            ys, xs = slice(max(Y - r, 0), min(Y + r, H - 1) + 1), slice(max(X - r, 0), min(X + r, W - 1) + 1)
            ma, mb = a[ys, xs].reshape(-1, 3).mean(axis=0), b[ys, xs].mean()
            q[Y, X] = sum(ma[c] * (I8[Y, X, c] / 255.0) for c in range(3)) + mb
    return np.clip(q, 0, 1).astype(np.float32)


@pytest.mark.parametrize('r,eps', [(1, 1e-6), (2, 1e-4), (5, 1e-2), (20, 1e-4)])
def test_oracle_against_brute_force(r, eps):
    I8 = AO.make_photo(7, 9, 12)
    rng = np.random.RandomState(3)
    p8 = np.zeros((9, 12), np.uint8)
    p8[2:7, 3:10] = 255
    p8[4:6, 1:8] = rng.randint(0, 256, (2, 7))
    got, want = MO.guided_matte(I8, p8, r, eps), _brute(I8, p8, r, eps)
    # both are float64 evaluations of the same rationals; they differ by the order of the sums and the solver: the 3 x 3 system has a
    # condition number of at most 0.25 / eps, so 1e-16 * 2.5e5 * |a| stays below 1e-8; one float32 ulp at 1 is 6e-8
    assert np.abs(got.astype(np.float64) - want).max() <= 1.2e-7


@pytest.mark.parametrize('c', [0, 1, 77, 255])
def test_constant_weight_is_reproduced_exactly(c):
    I8 = AO.make_photo(8, 23, 31)
    for r in (1, 4, 40):
        m = MO.guided_matte(I8, np.full((23, 31), c, np.uint8), r, 1e-4)
        assert (m == np.float32(c / 255.0)).all()


def test_flat_guide_gives_box_mean_of_box_mean():
    rng = np.random.RandomState(4)
    p8 = rng.randint(0, 256, (17, 22)).astype(np.uint8)
    I8 = np.full((17, 22, 3), (90, 14, 201), np.uint8)
    for r in (1, 3, 30):
        n = MO.box(np.ones(p8.shape, np.int64), r).astype(np.float64)
        b = (MO.box(p8.astype(np.int64), r) / (255.0 * n)).astype(np.float32).astype(np.float64)        # a = 0 exactly
        want = np.clip(MO.box(b, r) / n, 0, 1).astype(np.float32)
        assert np.array_equal(MO.guided_matte(I8, p8, r, 1e-4), want)


def test_weight_that_is_a_guide_channel_is_reproduced():
    I8 = AO.make_photo(9, 40, 52)
    for r in (1, 3, 8):
        m = MO.guided_matte(I8, I8[..., 1], r, 1e-9)
        assert np.abs(m.astype(np.float64) - I8[..., 1] / 255.0).max() <= 1e-3


def test_int32_bound_at_max_radius():
    r = AL.MATTE_MAX_RADIUS
    assert r == 64 and 255 * 255 * (2 * r + 1) ** 2 < 2 ** 31 <= 255 * 255 * (2 * 91 + 1) ** 2       # int32 would hold up to r = 90
    I8 = np.full((2 * r + 1, 2 * r + 1, 3), 255, np.uint8)
    n, sp, sI, sIp, sII = MO.moments(I8, np.full(I8.shape[:2], 255, np.uint8), r)
    assert n[r, r] == (2 * r + 1) ** 2 and sII.max() == sIp.max() == 255 * 255 * (2 * r + 1) ** 2 < 2 ** 31


def test_matte_params_defaults_and_errors():
    assert AL.matte_params(True, 0.43) == (10, 1e-4)            # ceil(4 / 0.43)
    assert AL.matte_params({}, 3.2) == (2, 1e-4)
    assert AL.matte_params(True, 8.0) == (1, 1e-4)
    assert AL.matte_params(True, 0.01) == (64, 1e-4)
    assert AL.matte_params({'radius': 7}, 0.1) == (7, 1e-4)
    assert AL.matte_params({'eps': 1e-2}, 1.0) == (4, 1e-2)
    assert AL.matte_params({'radius': 64, 'eps': 1e-6}, 1.0) == (64, 1e-6)
    for bad in ({'radius': 0}, {'radius': 65}, {'radius': 2.5}, {'eps': 0.0}, {'eps': -1e-4}, {'eps': float('nan')}, {'eps': float('inf')},
                {'size': 3}, False, 'on'):
        with pytest.raises(ValueError):
            AL.matte_params(bad, 1.0)


def test_cases_cover_the_grid():
    got = set(MC.CASES.values())
    for plan in ('e_batch_feather', 'b_minify', 'c_padded', 'f_origin'):
        for r in (1, 3, 8):
            for eps in (1e-2, 1e-4):
                assert (plan, r, eps) in got
    assert any(r == 64 for _, r, _ in got) and MC.CASES[MC.WORST][1:] == (1, 1e-6)
    c = MC.inputs('e_batch_feather-r64-eps0.0001')
    x0, y0, x1, y1 = c['plan_u']['bbox']
    assert max(x1 - x0, y1 - y0) <= 2 * 64, 'at r = 64 every window must be clipped by the domain'
    w = c['weight']
    assert (w == 255).any() and (w[: w.shape[0] // 5] == 0).all() and ((w > 0) & (w < 255)).any()


def test_float32_moments_miss_half_a_grey_level():
    """Why the moments are integers: window means formed in float32 and subtracted lose the covariance's low bits, and at eps = 1e-6
    the solve amplifies that beyond half a grey level of alpha (1 / 510) on the worst case; the exact-integer oracle is the yardstick."""
    c = MC.inputs(MC.WORST)
    _, alpha = MC.oracle(MC.WORST)
    _, alpha32 = MO.paste_back_matte(c['photo'], c['edits'][:1], c['plan_u'], c['weight'], c['feather'], c['radius'], c['eps'], moments_mode='f32')
    d = float(np.abs(alpha.astype(np.float64) - alpha32).max())
    print(f'float32 moments: max |alpha - alpha_f32| = {d:.3e}')
    assert d > 1.0 / 510.0


def test_uncrop_job_labels_and_matte_arguments(tmp_path, capsys):
    """dataset uncrop: --matte without --labels is an argument error; with a label directory the job hands paste_back the hair of the
    label PNG as a 255 / 0 weight (resized nearest to the crop's side) and the matte parameters."""
    from PIL import Image
    from ctrlhair_amd import dataset as DS
    from ctrlhair_amd.hostutil import HAIR_IDX
    for extra in (['--matte'], ['--matte-radius', '3'], ['--matte-eps', '1e-3']):
        with pytest.raises(SystemExit) as e:
            DS._main_uncrop(['p', 'e', 'o', '--landmarks', 'x'] + extra)
        assert e.value.code == 2 and '--labels' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        DS._main_uncrop(['p', 'e', 'o', '--landmarks', 'x', '--labels', 'l', '--matte-radius', '65'])
    with pytest.raises(ValueError, match='label_dir'):
        DS.uncrop_faces(None, 'p', 'e', str(tmp_path / 'o'), '', {}, matte=True)

    for d in ('photos', 'edits', 'labels'):
        (tmp_path / d).mkdir()
    photo = AO.make_photo(3, 90, 110)
    Image.fromarray(photo).save(tmp_path / 'photos' / 'a.png')
    Image.fromarray(photo).save(tmp_path / 'photos' / 'b.png')            # no label map: skipped
    for n in ('a.png', 'b.png'):
        Image.fromarray(AO.make_photo(4, 16, 16)).save(tmp_path / 'edits' / n)
    lab = np.zeros((8, 8), np.uint8)
    lab[2:5, 1:7] = HAIR_IDX
    lab[6, 6] = 1
    Image.fromarray(lab).save(tmp_path / 'labels' / 'a.png')
    want = np.kron((lab == HAIR_IDX).astype(np.uint8) * 255, np.ones((2, 2), np.uint8))
    assert np.array_equal(DS.label_weight(str(tmp_path / 'labels' / 'a.png'), 16), want)
    calls = []

    class Aligner:
        def paste_back(self, photo, edit, plan, weight=None, matte=None):
            import torch
            calls.append((weight, matte, plan['output_size']))
            return torch.from_numpy(photo[None].copy())

    lm = {n: AO.make_landmarks(5, (55.0, 40.0), 12.0, 4.0) for n in ('a.png', 'b.png')}
    done, skipped = DS.uncrop_faces(Aligner(), str(tmp_path / 'photos'), str(tmp_path / 'edits'), str(tmp_path / 'out'), '', lm,
                                    label_dir=str(tmp_path / 'labels'), matte={'radius': 3})
    assert done == ['a.png'] and skipped == ['b.png'] and len(calls) == 1
    assert np.array_equal(calls[0][0], want) and calls[0][1] == {'radius': 3} and calls[0][2] == 16
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'out' / 'a.png')), photo)
