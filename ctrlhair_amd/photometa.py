"""What a photo file says about itself besides its pixels: EXIF orientation, the EXIF block to carry over, the ICC profile.

All three come from Pillow's lazy open -- `Image.open` reads the headers and decodes no pixels -- and the EXIF to carry over is exactly
what `ImageOps.exif_transpose` leaves behind: the Exif object with the orientation tag deleted, serialised by Pillow.  The host path
(dataset.read_rgb(orient=True), which calls exif_transpose) and the device path (which calls read_metadata on the file's bytes and turns
the pixels with ch_orient_u8) therefore write the same metadata bytes by construction; there is no TIFF / IFD parser here.

Imports neither torch nor the library.
"""
import io
from typing import Optional, Tuple

ORIENTATION_TAG = 0x0112
Metadata = Tuple[int, Optional[bytes], Optional[bytes]]
NONE: Metadata = (1, None, None)
EXIF_MAX = 65533                          # longest EXIF block one JPEG APP1 segment holds (the 2-byte length counts itself); Pillow's
                                          # save() raises ValueError('EXIF data is too long') above it


def turns(orientation) -> bool:
    """True for 2..8: the EXIF orientations that change the pixels.  1, a missing tag and anything outside 1..8 leave the image alone."""
    return isinstance(orientation, int) and not isinstance(orientation, bool) and 2 <= orientation <= 8


def image_metadata(im, strip: bool = True) -> Metadata:
    """(orientation, exif bytes or None, icc profile or None) of an opened PIL image, before any transpose.  The orientation is the tag's
    value as stored (values outside 1..8 mean 'leave alone' to every consumer here).  The EXIF bytes are what ImageOps.exif_transpose
    leaves in info['exif']: for an orientation that turns the pixels (2..8) Pillow's serialisation of the Exif object without the tag;
    for any other value, and without strip (the pixels stay as stored, so the tag stays true), the file's own block untouched.  None
    for a file without EXIF.  The image's own Exif object is left as it was found."""
    exif = im.getexif()
    stored = exif.get(ORIENTATION_TAG, 1)
    orientation = int(stored) if isinstance(stored, int) else 1
    data = None
    if len(exif) > 0:                       # a file without an EXIF block carries none over (exif_transpose adds none either)
        if strip and turns(orientation):
            del exif[ORIENTATION_TAG]       # the object is the image's own (getexif caches it): put the tag back for a later exif_transpose
            try:
                data = exif.tobytes()
            finally:
                exif[ORIENTATION_TAG] = stored
        else:
            data = im.info.get('exif') or exif.tobytes()
            data = bytes(data)
    icc = im.info.get('icc_profile')
    return orientation, data, (bytes(icc) if icc else None)


def read_metadata(data, strip: bool = True) -> Metadata:
    """(orientation, exif_bytes_or_None, icc_or_None) from a file's bytes, or from a path (str / os.PathLike): image_metadata of Pillow's
    lazy open, which reads the headers only and decodes no pixels.  Never raises: a file Pillow cannot open, or whose EXIF it cannot
    read, gives (1, None, None)."""
    import os
    from PIL import Image
    try:
        with Image.open(data if isinstance(data, (str, os.PathLike)) else io.BytesIO(data)) as im:
            return image_metadata(im, strip)
    except Exception:
        return NONE


def per_image(values, N: int, what: str) -> list:
    """The per-image metadata argument of the encoders as a list of N: None -> N times None; a list of N bytes-or-None is checked."""
    if values is None:
        return [None] * N
    if isinstance(values, (bytes, bytearray)) or len(values) != N:
        raise ValueError(f'{what} must be a list of one bytes object or None per image ({N})')
    return list(values)


def droppable(exif: Optional[bytes], what: str = '') -> Optional[bytes]:
    """exif, or None with a printed warning when it is too long for one JPEG APP1 segment (Pillow's save() refuses such a block; both
    writers of the crop jobs drop it instead, alike)."""
    if exif is not None and len(exif) > EXIF_MAX:
        print(f'warning: {what + ": " if what else ""}EXIF block of {len(exif)} bytes does not fit one APP1 segment, dropped')
        return None
    return exif
