"""Oracle vs the reference's generator module on inputs no other fixture uses: the reference's outputs are stored in
tests/golden/oracle_vs_reference_fresh.npz (written by tests/golden/make_golden.py fresh from the imported reference)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.mark.parametrize('B,ui,seed', [(2, False, 100), (1, True, 200)])
def test_generator_fresh_inputs(B, ui, seed):
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    ngf, S = 16, 64
    z = np.load(os.path.join(GOLDEN, 'oracle_vs_reference_fresh.npz'))
    key = f'{B}_{int(ui)}_{seed}'
    sd = P.sean_state_dict(0, ngf)
    lab = P.blocky_labels(B, S, seed=seed, grid=4)
    assert np.array_equal(lab, z['labels_' + key])          # the fixture was made on these very inputs
    codes = P.style_codes(B, seed=seed + 1)
    nz = P.noise_planes(B, S, ngf, seed=seed + 2)
    ref = z['image_' + key]
    mine = O.generator_forward(O.to_torch(sd), lab, codes, nz, ngf).numpy()
    assert np.abs(ref - mine).max() <= 1e-5
