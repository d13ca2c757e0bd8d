"""Record tests/golden/jpeg_golden.npz: Pillow's JPEG file bytes for every case of tests/jpeg_cases.py, so that the tests do not depend
on the Pillow build of the machine they run on.  One array of bytes per case id, plus 'pillow' / 'libjpeg' (the versions recorded from).

    python tools/jpeg_golden.py [--out tests/golden/jpeg_golden.npz]
"""
import argparse
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import PIL
    from PIL import Image, features
    from tests import jpeg_cases as JC
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'jpeg_golden.npz'))
    args = ap.parse_args()
    out = {'pillow': np.array(PIL.__version__), 'libjpeg': np.array(str(features.version('jpg')))}
    for case in JC.CASES:
        buf = io.BytesIO()
        Image.fromarray(JC.case_image(case)).save(buf, 'JPEG', quality=case[3], subsampling=JC.SUBSAMPLING[case[4]])
        out[JC.case_id(case)] = np.frombuffer(buf.getvalue(), np.uint8)
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {len(JC.CASES)} files, {sum(v.size for k, v in out.items() if k not in ("pillow", "libjpeg"))} bytes, '
          f'{os.path.getsize(args.out)} on disk')


if __name__ == '__main__':
    main()
