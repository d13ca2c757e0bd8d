"""Records the reference's median style codes -> tests/golden/medoid_golden.npz.  Build-container only (run from the repository root:
`python tests/golden/make_medoid_golden.py`): it writes the golden input of tests/medoid_oracle.py as the tree the reference reads,
styles_test/style_codes/<img>/<i>/ACE.npy in a temporary directory, runs the reference's own sean_codes/get_mean_code.py there with
runpy (the script works relative to the current directory), and reads back styles_test/mean_style_code/median/<i>/ACE.npy.

The file holds only `rows` (float32 [19,512]: the chosen code per region, zeros where the reference wrote none), `written` (bool [19]),
`index` (which image each row came from, -1 where none) and `presence` (bool [24,19]); the inputs are regenerated from their seeds.

The reference sums float32 Gram-identity distances, so its choice is only meaningful where the runner-up is far enough away: the script
asserts that every region's float64 runner-up gap exceeds 1e-3 relative (the reference's error on this family is ~5e-6)."""
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from refharness import REF                 # noqa: E402  (where the reference checkout lies)

from tests import medoid_oracle as O       # noqa: E402

MIN_GAP = 1e-3


def main():
    codes, pres = O.golden_codes(), O.golden_presence()
    N, R, D = codes.shape
    count = pres.sum(axis=0)
    assert count[O.GOLDEN_ONE] == 1 and count[O.GOLDEN_NONE] == 0 and len(set(count.tolist())) > 4, count
    index64, count64, _, gaps = O.median_rows_f64(codes)
    assert (count64 == count).all()
    for j in range(R):
        print(f'region {j:2d}: count {count[j]:2d}  f64 medoid image {index64[j]:2d}  runner-up gap {gaps[j]:.3e}')
        assert count[j] <= 1 or gaps[j] > MIN_GAP, (j, gaps[j])
    rows, written, index = np.zeros((R, D), np.float32), np.zeros(R, bool), np.full(R, -1, np.int64)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(N):
            for j in range(R):
                if pres[i, j]:
                    d = os.path.join(tmp, 'styles_test', 'style_codes', f'img{i:03d}', str(j))
                    os.makedirs(d)
                    np.save(os.path.join(d, 'ACE.npy'), codes[i, j])
        os.chdir(tmp)
        try:
            runpy.run_path(os.path.join(REF, 'sean_codes', 'get_mean_code.py'), run_name='__main__')
        finally:
            os.chdir(cwd)
        for j in range(R):
            p = os.path.join(tmp, 'styles_test', 'mean_style_code', 'median', str(j), 'ACE.npy')
            if os.path.exists(p):
                rows[j], written[j] = np.load(p), True
                hit = np.nonzero((codes[:, j] == rows[j]).all(axis=1))[0]
                assert len(hit) == 1, (j, hit)
                index[j] = hit[0]
    assert (written == (count > 0)).all()
    assert (index == index64).all(), (index, index64)        # glob order differs from ours; the chosen code does not
    path = os.path.join(HERE, 'medoid_golden.npz')
    np.savez_compressed(path, rows=rows, written=written, index=index, presence=pres)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
