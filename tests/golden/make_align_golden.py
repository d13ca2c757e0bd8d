"""Records the reference's face alignment -> tests/golden/align_golden.npz.  Build-container only (run from the repository root:
`python tests/golden/make_align_golden.py`): it imports external_code/crop.py::recreate_aligned_images from the reference checkout
where it lies and runs it on the seeded photos and landmarks of tests/align_oracle.py (nothing of the inputs is stored but their
SHA-256).  Two shims make the import work with today's libraries: PIL.Image.ANTIALIAS (removed in Pillow 10; it was LANCZOS) and a
stub `cv2` whose getPerspectiveTransform is this project's numpy solve (cv2 is not installed; the 8x8 solve is not bit-equal to
OpenCV's, which only matters for a landmark that falls exactly on a rounding boundary).

Per case the file holds `<name>/crop` (uint8 [S,S,3]; for the 512- and 1024-px cases, which would not fit the size limit, the 256 x 256
centre window as `<name>/window` instead), `<name>/crop_sha256`, `<name>/landmarks` int32 [68,2], `<name>/photo_sha256`,
`<name>/lm_sha256` and `<name>/branches` = (shrink, cropped, padded) as the reference took them."""
import os
import sys
import types

import numpy as np
import PIL.Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from refharness import REF                 # noqa: E402  (where the reference checkout lies)

from ctrlhair_amd import alignment as A      # noqa: E402
from tests import align_oracle as O          # noqa: E402

# what each case must exercise: (shrink > 1, cropped, padded)
EXPECT = {'plain_256': (False, True, False), 'pad_topleft_512': (False, True, True), 'shrink_256': (True, True, False),
          'shrink_pad_256': (True, True, True), 'nocrop_1024': (False, False, False), 'pad_right_1024': (False, True, True)}
WINDOW = 256


def reference_fn():
    if not hasattr(PIL.Image, 'ANTIALIAS'):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    cv2 = types.ModuleType('cv2')
    cv2.getPerspectiveTransform = lambda src, dst: A.perspective_matrix(src, dst)
    sys.modules['cv2'] = cv2
    sys.path.insert(0, REF)
    from external_code.crop import recreate_aligned_images
    return recreate_aligned_images


class Spy:
    """Notes which branches the reference takes, by watching the PIL / numpy calls it makes."""

    def __init__(self):
        self.resizes, self.crops, self.pads = [], 0, 0

    def __enter__(self):
        spy = self
        self._resize, self._crop, self._pad = PIL.Image.Image.resize, PIL.Image.Image.crop, np.pad

        def resize(im, size, *a, **k):
            spy.resizes.append((im.size, tuple(size)))
            return spy._resize(im, size, *a, **k)

        def crop(im, *a, **k):
            spy.crops += 1
            return spy._crop(im, *a, **k)

        def pad(*a, **k):
            spy.pads += 1
            return spy._pad(*a, **k)
        PIL.Image.Image.resize, PIL.Image.Image.crop, np.pad = resize, crop, pad
        return self

    def __exit__(self, *exc):
        PIL.Image.Image.resize, PIL.Image.Image.crop, np.pad = self._resize, self._crop, self._pad


def main():
    ref = reference_fn()
    out = {}
    for name in O.CASES:
        photo, lm, S, T = O.case_inputs(name)
        with Spy() as spy:
            img, pts = ref(photo.copy(), lm.copy(), output_size=S, transform_size=T)
        crop = np.asarray(img)
        assert crop.shape == (S, S, 3) and crop.dtype == np.uint8
        shrunk = any(src != (T, T) for src, _ in spy.resizes)            # a resize that is not the final reduction
        took = (shrunk, spy.crops > 0, spy.pads > 0)
        assert took == EXPECT[name], (name, took, EXPECT[name])
        if S <= 256:
            out[f'{name}/crop'] = crop
        else:
            o = (S - WINDOW) // 2
            out[f'{name}/window'] = crop[o:o + WINDOW, o:o + WINDOW]
        out[f'{name}/crop_sha256'] = np.array(O.sha256(crop))
        out[f'{name}/landmarks'] = np.asarray(pts, np.int32)
        out[f'{name}/photo_sha256'] = np.array(O.sha256(photo))
        out[f'{name}/lm_sha256'] = np.array(O.sha256(lm))
        out[f'{name}/branches'] = np.array(took)
        print(name, 'branches', took, 'crop mean', float(crop.mean()))
    seen = np.array([EXPECT[n] for n in O.CASES])
    assert seen.any(0).all() and (~seen).any(0).all()
    assert {O.CASES[n][6] for n in O.CASES} >= {256, 512, 1024}
    path = os.path.join(HERE, 'align_golden.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != 'align_golden.npz')
    print(path, size, 'bytes')
    assert size < min(largest, 1 << 20), size


if __name__ == '__main__':
    main()
