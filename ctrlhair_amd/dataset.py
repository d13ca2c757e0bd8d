"""Dataset-scale mask extraction and SEAN style-code encoding.

The reference walks a directory one image at a time (dataset_scripts/script_get_mask.py:55-71 -> `label/<name>.png`,
dataset_scripts/script_get_sean_code.py:40-62 -> `sean_code/<dataset>___<name>.pkl` merged into `sean_code_dict.pkl` by
dataset_scripts/utils.py:14-21).  Here the same BiSeNet / Zencoder kernels run over batches, and the file list is
sharded over ranks (one process per GPU; no collective on the data path -- rank r owns files r, r+W, r+2W, ...).

On-disk formats are the reference's:
  label/<name>.png                      8-bit single-channel PNG, CelebAMask-HQ ids, 512x512 (script_get_mask.py:44-50)
  sean_code/<dataset>___<name>.pkl      pickle of float32 [19,512] (script_get_sean_code.py:56-62)
  sean_code_dict.pkl                    pickle of {'<dataset>___<name>': float32 [19,512]} (utils.py:14-21)
  images_256/<name>                     the aligned portrait under the source photo's file name (script_crop.py:31-54)
  hair_info_all_dataset/rgb_stat/<dataset>___<name>.pkl        [moment1..4], float64 [3] each (script_get_rgb_hsv_label.py:58-67)
  hair_info_all_dataset/color_var_stat/<dataset>___<name>.pkl  {'var_rgb', 'var_hsv', 'var_pca', 'var_pca_mean', 'var_pca_comp'},
                                        only for images with > 5 hair pixels (script_get_color_var_label.py:58-90)
  rgb_stat_dict.pkl, color_var_stat_dict.pkl   the merged dicts;  hsv_stat_dict_ordered.pkl   uint8 [N,3] table of the colour
                                        sliders (script_get_rgb_hsv_label.py:70-90; load with hostutil.DistTranslation(root=<root>))

    python -m ctrlhair_amd.dataset masks    <root> <dataset> [--batch 16] [--png host|device] [--decode host|device]
    python -m ctrlhair_amd.dataset codes    <root> <dataset> [--batch 16] [--decode host|device]
    python -m ctrlhair_amd.dataset rgb      <root> <dataset> [--batch 16]     (no network weights: ctrlhair_amd.colorstats)
    python -m ctrlhair_amd.dataset colorvar <root> <dataset> [--batch 16]
    python -m ctrlhair_amd.dataset crop <src_dir> <root> <dataset> --landmarks <file> [--size 256] [--png host|device]
                                          [--jpeg host|device] [--jpeg-quality 75] [--jpeg-subsampling 420|444] [--decode host|device]
                                          (dataset_scripts/script_crop.py: FFHQ-align every photo of <src_dir> into
                                           <root>/<dataset>/images_256/<name>; no network weights: ctrlhair_amd.alignment)
    python -m ctrlhair_amd.dataset uncrop <photos> <edits> <out> --landmarks <file> [--size S]
                                          [--labels DIR [--matte] [--matte-radius R] [--matte-eps E]] [--png host|device]
                                          [--jpeg host|device] [--jpeg-quality 75] [--jpeg-subsampling 420|444] [--decode host|device]
                                          (the inverse of crop: paste the edited crop <edits>/<name> back into <photos>/<name> with the
                                           same landmarks and write the photo-sized result to <out>/<name>; ctrlhair_amd.alignment.
                                           --labels: 8-bit label PNGs <DIR>/<stem>.png of the crops; only their hair is pasted, and with
                                           --matte that region is refined by a guided filter of the photo: ch_face_unalign_matte)
    python -m ctrlhair_amd.dataset median <root> [--out FILE] [--tree DIR]
                                          (sean_codes/get_mean_code.py: the per-region medoid of <root>/sean_code_dict.pkl, written as
                                           <root>/mean_style_code.npz for HairEditor(mean_style_code=...); no network weights:
                                           ctrlhair_amd.stylestats.  Single process: all 19 regions are one kernel call that takes
                                           well under a second at tens of thousands of images, so there is nothing to shard)
    python -m ctrlhair_amd.dataset warp-pool <root> <pool_dir> --landmarks <file> (--pairs N [--seed S] | --pairs-file FILE)
                                          [--datasets A B ...] [--batch 16] [--only-hair]
                                          (shape_branch/adaptor_generation.py AdaptorPoolGeneration: warp the hair mask of
                                           <root>/<hair dataset>/label/<hair name>.png onto <root>/<face dataset>/label/<face name>.png
                                           for many hair / face pairs and write <pool_dir>/<hair_dir>___<hair_num>___<face_dir>___
                                           <face_num>___<rank:02d>.png; landmarks: name -> [81,2] in [0,1]; meshing and warp are
                                           batched on the GPU: warping.MaskWarper.warp_batch(mesher='device'))
    python -m ctrlhair_amd.dataset directions <img_dir> --att shape|texture [--weights procedural|<checkpoint root>] [--used-dir DIR]
                                          [--out DIR] [--n 300] [--images 10] [--values 6] [--max-val 2.5] [--seed 0] [--noise-seed 0]
                                          [--size 256|512] [--cell PX] [--sheets all|top:K|none] [--list FILE] [--batch 16]
                                          [--png host|device] [--png-stride]
                                          (shape_branch/ and color_texture_branch/script_find_direction.py: random candidate directions
                                           orthogonal to the ones in <used-dir>, each swept over the first --images images of <img_dir> (or
                                           the names in --list) at --values slider values; writes <out>/<att>_dir_<k+1>/<i>.pkl,
                                           <out>/<att>_<k+1>/<i>.png and <out>/scores.json, k = the number of directions in use;
                                           candidates are sharded over ranks: ctrlhair_amd.directions)
    python -m ctrlhair_amd.dataset use-direction <out> <att> <index> <used-dir>
                                          (copy candidate <index> of that search into the used set under the next free name)
    (masks, crop, uncrop and directions take --png host|device: 'device' encodes their PNG files with ch_png_encode,
     ctrlhair_amd.pngenc, instead of downloading the pixels for Pillow; the pixels are the same, the file bytes are not;
     directions --png device --png-stride: the encoder also matches at the sheet's column pitch (ch_png_encode_dist): smaller sheets)
    (crop and uncrop take --jpeg host|device for their .jpg / .jpeg names: 'device' encodes them with ch_jpeg_encode,
     ctrlhair_amd.jpegenc, instead of downloading the pixels for Pillow; the FILES are the same, byte for byte, as Pillow's at the same
     --jpeg-quality and --jpeg-subsampling, whose defaults 75 and 420 are what Pillow's save() uses when given neither; .bmp stays Pillow's)
    (crop and uncrop take --decode host|device for the photos and edits they read: 'device' uploads the files' bytes and decodes them
     there, .jpg / .jpeg with ch_jpeg_decode (ctrlhair_amd.jpegdec), .png with ch_png_decode; the pixels are Pillow's, so the results are
     the same files; progressive JPEGs and whatever else the device does not take are decoded by Pillow, file by file)
    (crop and uncrop take --orient [--landmark-frame upright|stored] and --metadata drop|keep: --orient makes every photo upright by its
     EXIF orientation before it is aligned or pasted into -- Pillow's exif_transpose on the host, ch_orient_u8 (ctrlhair_amd.orient) with
     --decode device, the same pixels -- and takes the landmarks as pixels of the upright photo, or of the stored one with
     --landmark-frame stored; --metadata keep writes the photo's ICC profile and its EXIF block, without the orientation tag where the
     pixels were made upright, into the output, whoever writes it.  Without them nothing changes: the stored pixels, no metadata)
    (masks and codes take --decode host|device too: 'device' decodes a batch's files in the same way and then resizes and normalises them
     there in one call, ch_ingest_images / ch_ingest_labels (ctrlhair_amd.ingest): the networks see the same tensors bit for bit)
    (under torch.distributed.run for several GPUs; RANK / WORLD_SIZE / LOCAL_RANK are read from the environment)
"""
import os
import pickle
from typing import Dict, Iterable, List, Sequence

import numpy as np

from .photometa import turns as photometa_turns      # (host code: no torch, no library)

IMG_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


# ---- host logic (no GPU) ---------------------------------------------------------------------------------------------
def list_images(img_dir: str) -> List[str]:
    """Sorted image file names of a directory (script_get_sean_code.py:30-35 sorts the joined list)."""
    return sorted(f for f in os.listdir(img_dir) if f.lower().endswith(IMG_EXT))


def shard(items: Sequence, rank: int, world: int) -> List:
    """Round-robin shard of a sorted list: equal sizes up to one item, independent of the batch size."""
    if not 0 <= rank < world:
        raise ValueError(f'rank {rank} outside world {world}')
    return list(items[rank::world])


def batches(items: Sequence, n: int) -> Iterable[List]:
    for i in range(0, len(items), n):
        yield list(items[i:i + n])


def code_key(dataset: str, file_name: str) -> str:
    """'%s___%s' % (dataset_name, base_name[:-4])  (script_get_sean_code.py:60)."""
    return '%s___%s' % (dataset, os.path.splitext(file_name)[0])


def merge_pickle_dir_to_dict(dir_name: str, target_path: str) -> Dict[str, np.ndarray]:
    """dataset_scripts/utils.py:14-21."""
    res = {}
    for f_name in sorted(os.listdir(dir_name)):
        if f_name.endswith('.pkl'):
            with open(os.path.join(dir_name, f_name), 'rb') as f:
                res[f_name[:-4]] = pickle.load(f)
    with open(target_path, 'wb') as f:
        pickle.dump(res, f)
    return res


def read_rgb(path: str, orient: bool = False, metadata: bool = False):
    """The file's pixels as uint8 [H,W,3].  orient: made upright by ImageOps.exif_transpose (EXIF orientation 2..8; anything else leaves
    them alone).  metadata: -> (pixels, (orientation, exif bytes or None, icc profile or None)), photometa.image_metadata's triple: the
    EXIF block is the one that belongs to the returned pixels, without the orientation tag when they were made upright, with it else."""
    from PIL import Image
    im = Image.open(path)
    if not orient and not metadata:
        return np.asarray(im.convert('RGB'))
    from PIL import ImageOps
    from . import photometa
    from .orient import turns
    try:
        meta = photometa.image_metadata(im, strip=orient)
    except Exception:                                       # as read_metadata: EXIF that Pillow cannot read is no metadata, and no turn
        meta = photometa.NONE
    pixels = np.asarray((ImageOps.exif_transpose(im) if orient and turns(meta[0]) else im).convert('RGB'))
    return (pixels, meta) if metadata else pixels


def read_gray(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert('L'))


def write_label_png(path: str, label: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.asarray(label, dtype=np.uint8), mode='L').save(path)


# ---- batched drivers (HairEditor on the HIP library) -----------------------------------------------------------------
def _png_encoder(png: str, owner):
    """None for png='host'; for 'device' the device encoder (pngenc.PngEncoder) on `owner`'s handle and device.  The option names who
    writes PNG files: a .jpg name of the crop jobs follows the jpeg option (_jpeg_writer), any other format is Pillow's either way."""
    from .pngenc import PngEncoder, check_png_mode
    return PngEncoder(owner.handle, owner.device) if check_png_mode(png) == 'device' else None


def _jpeg_writer(jpeg: str, quality, subsampling, owner):
    """(encoder, save_options) for the .jpg / .jpeg names of the crop jobs.  jpeg='host': (None, options) -- Pillow writes the file, with
    no options at all while quality and subsampling are at their defaults (75, 4:2:0: what save() then uses), so that nothing changes
    for callers that pass neither.  jpeg='device': (jpegenc.JpegEncoder on `owner`'s handle and device, options); the same file bytes."""
    from .jpegenc import JpegEncoder, check_jpeg_mode, check_jpeg_params
    quality, subsampling = check_jpeg_params(quality, subsampling)
    options = {'quality': quality, 'subsampling': subsampling}
    if check_jpeg_mode(jpeg) == 'device':
        return JpegEncoder(owner.handle, owner.device), options
    return None, ({} if (quality, subsampling) == (75, 2) else options)


def _png_decoder(decode: str, owner):
    """None for decode='host'; for 'device' the device decoder (pngdec.PngDecoder) on `owner`'s handle and device.  The option names
    who decodes the PNG files a job reads; whatever the device does not decode is Pillow's, file by file (PngDecoder.fallbacks)."""
    from .pngdec import PngDecoder, check_decode_mode
    return PngDecoder(owner.handle, owner.device) if check_decode_mode(decode) == 'device' else None


class _PhotoReader:
    """read_rgb for the crop jobs with decode='device': .jpg / .jpeg files through jpegdec.JpegDecoder, .png files through
    pngdec.PngDecoder, on `owner`'s handle and device; anything else, and every file a decoder hands back, is Pillow's.  The pixels are
    device tensors and the same as read_rgb's; fallbacks counts the files Pillow decoded.
    orient: read_rgb / read_rgb_many make the pixels upright as dataset.read_rgb(orient=True) does: the files are decoded as stored, by
    the device or by Pillow, and those whose EXIF orientation is 2..8 are then turned by ONE orient.Orienter.apply call per batch.  The
    orientation, like the rest of the metadata, is photometa.read_metadata's, from Pillow's lazy open of the file (headers only)."""

    def __init__(self, owner, orient: bool = False):
        from .jpegdec import JpegDecoder
        from .pngdec import PngDecoder
        self.jpeg, self.png, self.other = JpegDecoder(owner.handle, owner.device), PngDecoder(owner.handle, owner.device), 0
        self.device = owner.device
        self.orient = bool(orient)
        self._owner, self._orienter = owner, None

    @property
    def fallbacks(self) -> int:
        return self.jpeg.fallbacks + self.png.fallbacks + self.other

    @property
    def orienter(self):
        """orient.Orienter on the owner's handle and device, made when the first photo is to be turned."""
        if self._orienter is None:
            from .orient import Orienter
            self._orienter = Orienter(self._owner.handle, self._owner.device)
        return self._orienter

    def _metadata(self, paths, orient: bool) -> List:
        """photometa.read_metadata per path: Pillow's lazy open of the file, which reads its headers and not the scan a decoder read."""
        from . import photometa
        return [photometa.read_metadata(p, strip=orient) for p in paths]

    def read_rgb(self, path: str, orient: bool = None, metadata: bool = False):
        """dataset.read_rgb(path, orient, metadata) with the pixels on the device; orient: default the reader's own."""
        import torch
        orient = self.orient if orient is None else bool(orient)
        if _is_jpeg(path):
            t = self.jpeg.read_rgb([path])[0]
        elif _is_png(path):
            t = self.png.read_rgb([path])[0]
        else:
            self.other += 1
            t = torch.from_numpy(np.array(read_rgb(path))).to(self.device)
        if not orient and not metadata:
            return t
        meta = self._metadata([path], orient)[0]
        if orient and photometa_turns(meta[0]):
            t = self.orienter.apply([t], [meta[0]])[0]
        return (t, meta) if metadata else t

    def _read_many(self, paths, gray: bool, orient: bool = False) -> List:
        import torch
        paths = list(paths)
        if orient:
            stored, orientations = self._read_many(paths, gray), [m[0] for m in self._metadata(paths, True)]
            return self.orienter.apply(stored, orientations) if any(photometa_turns(o) for o in orientations) else stored
        out = [None] * len(paths)
        for decoder, takes in ((self.jpeg, _is_jpeg), (self.png, _is_png)):
            idx = [i for i, p in enumerate(paths) if takes(p)]
            if idx:                                          # one call per decoder and batch; it counts its own fallbacks
                for i, t in zip(idx, (decoder.read_gray if gray else decoder.read_rgb)([paths[i] for i in idx])):
                    out[i] = t
        for i, p in enumerate(paths):
            if out[i] is None:
                self.other += 1
                out[i] = torch.from_numpy(np.array((read_gray if gray else read_rgb)(p))).to(self.device)
        return out

    def read_rgb_many(self, paths) -> List:
        """read_rgb of a batch, in the order of `paths`: one JpegDecoder call for its .jpg / .jpeg files and one PngDecoder call for its
        .png files (each groups equal sizes into one launch); uint8 device tensors [H,W,3].  A reader made with orient=True turns the
        whole batch's tagged files in one further launch."""
        return self._read_many(paths, gray=False, orient=self.orient)

    def read_gray_many(self, paths) -> List:
        """dataset.read_gray of a batch in the same way: uint8 device tensors [H,W]; only grey files are decoded on the device."""
        return self._read_many(paths, gray=True)


def _photo_reader(decode: str, owner, orient: bool = False):
    """None for decode='host' (dataset.read_rgb reads the photos); for 'device' a _PhotoReader on `owner`'s handle and device."""
    from .pngdec import check_decode_mode
    return _PhotoReader(owner, orient) if check_decode_mode(decode) == 'device' else None


LANDMARK_FRAMES = ('upright', 'stored')
METADATA_MODES = ('drop', 'keep')


def _check_photo_options(orient, landmark_frame: str, metadata: str) -> None:
    if landmark_frame not in LANDMARK_FRAMES:
        raise ValueError(f"landmark_frame must be 'upright' or 'stored', got {landmark_frame!r}")
    if metadata not in METADATA_MODES:
        raise ValueError(f"metadata must be 'drop' or 'keep', got {metadata!r}")


def _read_photo(reader, path: str, orient: bool, keep: bool):
    """(pixels, (orientation, exif, icc)) of a photo of the crop jobs: read_rgb of the host or of the device reader; with neither option
    the plain read of before and no metadata."""
    from . import photometa
    read = read_rgb if reader is None else reader.read_rgb
    if not orient and not keep:
        return read(path), photometa.NONE
    return read(path, orient=orient, metadata=True)


def _photo_landmarks(lm, meta, photo_shape, orient: bool, landmark_frame: str):
    """The landmarks in the frame of the pixels the job works on: with orient those are upright, and landmarks given for the stored
    pixels (landmark_frame='stored') move with them (orient.orient_points)."""
    from .orient import orient_points, turns, upright_shape
    if not orient or landmark_frame != 'stored' or not turns(meta[0]):
        return lm
    Hs, Ws = upright_shape(int(photo_shape[0]), int(photo_shape[1]), meta[0])      # the stored size: the turn's shape rule is its own inverse
    return orient_points(np.asarray(lm, np.float64), meta[0], Hs, Ws)


def _kept_metadata(meta, keep: bool, name: str) -> dict:
    """save() / encoder keywords of metadata='keep': the photo's ICC profile and the EXIF block that belongs to the job's pixels.  An
    EXIF block too long for a .jpg name's APP1 segment is dropped with a warning, whoever writes the file."""
    from . import photometa
    if not keep:
        return {}
    exif = photometa.droppable(meta[1], name) if _is_jpeg(name) else meta[1]
    return {k: v for k, v in (('exif', exif), ('icc_profile', meta[2])) if v}


def _is_png(name: str) -> bool:
    return name.lower().endswith('.png')


def _is_jpeg(name: str) -> bool:
    return name.lower().endswith(('.jpg', '.jpeg'))


def _image_ingest(reader, owner):
    """None without a reader (decode='host'); else ingest.ImageIngest on `owner`'s handle and device."""
    from .ingest import ImageIngest
    return None if reader is None else ImageIngest(owner.handle, owner.device)


def extract_masks(editor, img_dir: str, label_dir: str, batch: int = 16, rank: int = 0, world: int = 1,
                  parse_size: int = 512, png: str = 'host', decode: str = 'host', stats: dict = None) -> List[str]:
    """BiSeNet-parse every image of `img_dir` (this rank's shard) and write `label_dir/<name>.png`.
    Per image identical to FaceParsing.parsing_img + swap_parsing_label_to_celeba_mask (my_parsing_util.py:31-54).
    png='device': the label maps of a batch are encoded on the device in one call (the same pixels in another file).
    decode='device': the files of a batch are decoded on the device (.jpg / .jpeg: jpegdec.JpegDecoder, .png: pngdec.PngDecoder) and
    resized and normalised there in one call (ingest.ImageIngest.parse_input): the network sees the same float32 tensor bit for bit, so
    the label maps are the same; what a decoder does not take is Pillow's, file by file, and counted in stats['fallbacks'] when a dict
    is passed.  With png='device' as well the host touches file bytes only."""
    import torch
    from PIL import Image
    os.makedirs(label_dir, exist_ok=True)
    fp = editor.face_parsing
    encoder = _png_encoder(png, fp)
    reader = _photo_reader(decode, fp)
    ingest = _image_ingest(reader, fp)
    done = []
    for names in batches(shard(list_images(img_dir), rank, world), batch):
        if reader is not None:
            x = ingest.parse_input(reader.read_rgb_many([os.path.join(img_dir, n) for n in names]), parse_size, lut=fp.ingest_lut())
        else:
            x = torch.cat([fp.normalise(np.asarray(Image.fromarray(read_rgb(os.path.join(img_dir, n)))
                                                   .resize((parse_size, parse_size), Image.BILINEAR))) for n in names], dim=0)
        labels, _ = fp.parse_tensor(x)                       # uint8 [B,512,512], CelebAMask-HQ ids
        if encoder is not None:
            encoder.write([os.path.join(label_dir, os.path.splitext(n)[0] + '.png') for n in names], labels)
            done += names
            continue
        labels = labels.cpu().numpy()
        for n, lab in zip(names, labels):
            write_label_png(os.path.join(label_dir, os.path.splitext(n)[0] + '.png'), lab)
            done.append(n)
    if stats is not None:
        stats['fallbacks'] = 0 if reader is None else reader.fallbacks
    return done


def encode_sean_codes(editor, img_dir: str, label_dir: str, code_dir: str, dataset: str, batch: int = 16, rank: int = 0,
                      world: int = 1, decode: str = 'host', stats: dict = None) -> Dict[str, np.ndarray]:
    """Zencoder style codes of every (image, label) pair of this rank's shard -> `code_dir/<dataset>___<name>.pkl`.
    Per image identical to HairEditor.get_code(preprocess_img(img), preprocess_mask(label)) (hair_editor.py:121-157).
    decode='device': the image and label files of a batch are decoded on the device and brought to the network's size there
    (ingest.ImageIngest.sean_input / labels: the same tensors bit for bit); fallbacks to Pillow are counted in stats['fallbacks']."""
    import torch
    os.makedirs(code_dir, exist_ok=True)
    gen = editor.models.generator
    reader = _photo_reader(decode, gen)
    ingest = _image_ingest(reader, gen)
    out = {}
    for names in batches(shard(list_images(img_dir), rank, world), batch):
        if reader is not None:
            imgs = ingest.sean_input(reader.read_rgb_many([os.path.join(img_dir, n) for n in names]), editor.img_size)
            labs = ingest.labels(reader.read_gray_many([os.path.join(label_dir, os.path.splitext(n)[0] + '.png') for n in names]),
                                 editor.img_size)
            codes = gen.encode(imgs, labs).cpu().numpy()
        else:
            imgs = np.concatenate([editor.preprocess_img(read_rgb(os.path.join(img_dir, n))) for n in names], axis=0)
            labs = np.concatenate([editor.preprocess_mask(read_gray(os.path.join(label_dir, os.path.splitext(n)[0] + '.png')))[0]
                                   for n in names], axis=0)
            codes = gen.encode(torch.from_numpy(imgs.astype(np.float32)).to(editor.device),
                               torch.from_numpy(labs.astype(np.uint8)).to(editor.device)).cpu().numpy()
        for n, c in zip(names, codes):
            key = code_key(dataset, n)
            with open(os.path.join(code_dir, key + '.pkl'), 'wb') as f:
                pickle.dump(c, f)
            out[key] = c
    if stats is not None:
        stats['fallbacks'] = 0 if reader is None else reader.fallbacks
    return out


COLOR_JOBS = {'rgb': 'rgb_stat', 'colorvar': 'color_var_stat'}      # job -> hair_info_all_dataset/<dir>, <dir>_dict.pkl


def hair_color_stats(stats, img_dir: str, label_dir: str, out_root: str, dataset: str, jobs: Sequence[str] = ('rgb',),
                     batch: int = 16, rank: int = 0, world: int = 1, decode: str = 'host') -> Dict[str, Dict[str, object]]:
    """Hair colour labels of every (image, label) pair of this rank's shard (script_get_rgb_hsv_label.py:49-67,
    script_get_color_var_label.py:48-90): eroded hair mask and exact sums on the device (`stats`: colorstats.HairColorStats),
    statistics finished on the host, one pickle per image under `out_root/hair_info_all_dataset/<job dir>/`.  Returns
    {job: {key: value}}; the colorvar job has no entry (and writes no file) for images with <= 5 hair pixels.
    Images must be square: the reference resizes the label map to `hair_img.shape[:2]` as cv2's (w, h), which swaps the
    axes of a non-square image.
    decode='device': the image and label files of a batch are read as bytes and decoded on the device (pngdec.PngDecoder; the same
    pixels, so the same pickles byte for byte); the pixels are never on the host."""
    import torch
    from . import colorstats as CS
    unknown = [j for j in jobs if j not in COLOR_JOBS]
    if unknown:
        raise ValueError(f'unknown colour job(s) {unknown}; expected {sorted(COLOR_JOBS)}')
    decoder = _png_decoder(decode, stats)
    dirs = {j: os.path.join(out_root, 'hair_info_all_dataset', COLOR_JOBS[j]) for j in jobs}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    out = {j: {} for j in jobs}

    def flush(group):
        names, imgs, labs = zip(*group)
        sums = stats.sums(*((np.stack(imgs), np.stack(labs)) if decoder is None else (torch.stack(imgs), torch.stack(labs))))
        for n, sm in zip(names, sums):
            key = code_key(dataset, n)
            for j in jobs:
                v = CS.rgb_stat_from_sums(sm) if j == 'rgb' else CS.color_var_from_sums(sm)
                if v is None:
                    continue
                with open(os.path.join(dirs[j], key + '.pkl'), 'wb') as f:
                    pickle.dump(v, f)
                out[j][key] = v

    for names in batches(shard(list_images(img_dir), rank, world), batch):
        group = []
        if decoder is not None:
            dev_imgs = decoder.read_rgb([os.path.join(img_dir, n) for n in names])
            dev_labs = decoder.read_gray([os.path.join(label_dir, os.path.splitext(n)[0] + '.png') for n in names])
        for k, n in enumerate(names):
            img = read_rgb(os.path.join(img_dir, n)) if decoder is None else dev_imgs[k]
            if img.shape[0] != img.shape[1]:
                raise ValueError(f'{n}: image is {img.shape[1]}x{img.shape[0]}; the colour statistics need square images '
                                 f'(the reference\'s resize swaps (h, w) for cv2\'s dsize)')
            lab = read_gray(os.path.join(label_dir, os.path.splitext(n)[0] + '.png')) if decoder is None else dev_labs[k]
            if group and (group[-1][1].shape != img.shape or group[-1][2].shape != lab.shape):
                flush(group)             # one device batch per run of equal sizes
                group = []
            group.append((n, img, lab))
        if group:
            flush(group)
    return out


def merge_color_stats(out_root: str, jobs: Sequence[str]) -> None:
    """Rank 0 after the barrier: merge the per-image pickles (dataset_scripts/utils.py:14-21) and, for the rgb job, build
    hsv_stat_dict_ordered.pkl from the merged dict (script_get_rgb_hsv_label.py:70-90)."""
    from .colorstats import hsv_table
    for j in jobs:
        d = COLOR_JOBS[j]
        merged = merge_pickle_dir_to_dict(os.path.join(out_root, 'hair_info_all_dataset', d), os.path.join(out_root, d + '_dict.pkl'))
        if j == 'rgb':
            with open(os.path.join(out_root, 'hsv_stat_dict_ordered.pkl'), 'wb') as f:
                pickle.dump(hsv_table(merged), f)


def load_landmarks(path: str) -> Dict[str, np.ndarray]:
    """Landmarks of the crop job: image name -> float [68,2] (or [81,2]) PIXELS of the source photo.  `.npz` (one array per name) or
    a pickled dict, the container dataset_scripts/script_landmark_detection.py writes (landmark68.pkl; its values there are
    divided by the image height -- multiply them back before using them here).  A name may be the file name, the file name without
    its extension, or '<dataset>___<name without extension>' (the key layout of landmark68.pkl)."""
    if path.lower().endswith('.npz'):
        with np.load(path) as z:
            return {k: np.asarray(z[k], np.float64) for k in z.files}
    with open(path, 'rb') as f:
        d = pickle.load(f)
    if not isinstance(d, dict):
        raise ValueError(f'{path}: expected a dict of name -> [68,2] landmarks')
    return {str(k): np.asarray(v, np.float64) for k, v in d.items()}


def find_landmarks(landmarks: Dict[str, np.ndarray], dataset: str, file_name: str):
    for key in (file_name, os.path.splitext(file_name)[0], code_key(dataset, file_name)):
        if key in landmarks:
            return landmarks[key]
    return None


def crop_faces(aligner, src_dir: str, out_dir: str, dataset: str, landmarks: Dict[str, np.ndarray], size: int = 256, rank: int = 0,
               world: int = 1, png: str = 'host', jpeg: str = 'host', jpeg_quality: int = 75, jpeg_subsampling=2, decode: str = 'host',
               stats: dict = None, orient: bool = False, landmark_frame: str = 'upright', metadata: str = 'drop'):
    """dataset_scripts/script_crop.py:36-54 for this rank's shard of `src_dir`: align every photo that has landmarks
    (`aligner`: alignment.FaceAligner) and write it to `out_dir/<name>`.  Returns (done, skipped): the file names written and the
    ones without a landmark entry, which are reported and left out.  png='device': .png names are encoded on the device.  jpeg='device':
    .jpg / .jpeg names are encoded on the device, to the bytes Pillow writes at jpeg_quality and jpeg_subsampling (0 / '444' or
    2 / '420'); jpeg='host' passes those two to Pillow when they are not its defaults.  decode='device': the photos are decoded on the
    device (.jpg / .jpeg: jpegdec.JpegDecoder, .png: pngdec.PngDecoder; the same pixels, so the same files); what a decoder does not take
    is Pillow's, file by file, and counted in stats['fallbacks'] when a dict is passed.
    orient: every photo is made upright by its EXIF orientation before it is aligned, as a viewer (and a landmark detector that opens
    the file like one) sees it: ImageOps.exif_transpose on the host, orient.Orienter on the device, the same pixels.  The landmarks are
    then pixels of the upright photo; landmark_frame='stored': they are pixels of the stored photo and are moved along.
    metadata='keep': the photo's ICC profile and its EXIF block (with orient without the orientation tag) are written into the crop,
    by Pillow's save(exif=, icc_profile=) or by the device encoders, to the same bytes; 'drop': neither, as before."""
    from PIL import Image
    _check_photo_options(orient, landmark_frame, metadata)
    os.makedirs(out_dir, exist_ok=True)
    encoder = _png_encoder(png, aligner)
    jpeg_encoder, jpeg_options = _jpeg_writer(jpeg, jpeg_quality, jpeg_subsampling, aligner)
    reader = _photo_reader(decode, aligner)
    keep = metadata == 'keep'
    done, skipped = [], []
    for n in shard(list_images(src_dir), rank, world):
        lm = find_landmarks(landmarks, dataset, n)
        if lm is None:
            print(f'crop: no landmarks for {n}, skipped')
            skipped.append(n)
            continue
        photo, meta = _read_photo(reader, os.path.join(src_dir, n), orient, keep)
        lm = _photo_landmarks(lm, meta, photo.shape, orient, landmark_frame)
        crop, _ = aligner.align(photo, lm[:68], size)
        kept = _kept_metadata(meta, keep, n)
        lists = {k: [v] for k, v in kept.items()}
        if encoder is not None and _is_png(n):
            encoder.write([os.path.join(out_dir, n)], crop[None], **lists)
            done.append(n)
            continue
        if jpeg_encoder is not None and _is_jpeg(n):
            jpeg_encoder.write([os.path.join(out_dir, n)], crop[None], **jpeg_options, **lists)
            done.append(n)
            continue
        crop = crop.cpu().numpy() if hasattr(crop, 'cpu') else np.asarray(crop)
        Image.fromarray(crop).save(os.path.join(out_dir, n), **(jpeg_options if _is_jpeg(n) else {}), **kept)
        done.append(n)
    if stats is not None:
        stats['fallbacks'] = 0 if reader is None else reader.fallbacks
    return done, skipped


def label_weight(label_path: str, S: int) -> np.ndarray:
    """The paste-back weight of a crop's label PNG: uint8 [S,S], 255 on hair (HAIR_IDX), 0 elsewhere; a label map of another size is
    resized nearest, like everywhere labels meet images here."""
    from PIL import Image
    from .hostutil import HAIR_IDX
    lab = Image.open(label_path)
    if lab.mode not in ('L', 'P'):
        raise ValueError(f'{label_path}: expected an 8-bit single-channel label PNG, got mode {lab.mode}')
    if lab.size != (S, S):
        lab = lab.resize((S, S), Image.NEAREST)
    return ((np.asarray(lab) == HAIR_IDX) * 255).astype(np.uint8)


def uncrop_faces(aligner, photo_dir: str, edit_dir: str, out_dir: str, dataset: str, landmarks: Dict[str, np.ndarray], size: int = None,
                 rank: int = 0, world: int = 1, label_dir: str = None, matte=None, png: str = 'host', jpeg: str = 'host',
                 jpeg_quality: int = 75, jpeg_subsampling=2, decode: str = 'host', stats: dict = None, orient: bool = False,
                 landmark_frame: str = 'upright', metadata: str = 'drop'):
    """The inverse of crop_faces for this rank's shard of `photo_dir`: paste the edited crop `edit_dir/<name>` back into the photo
    `photo_dir/<name>` it was aligned from (same landmarks, same file names) and write the photo-sized result to `out_dir/<name>`.
    size: the crops' side (default: each edit's own).  label_dir: per-image weight from `label_dir/<stem>.png` (hair = 255); matte
    (True or a dict, alignment.matte_params; needs label_dir): that weight refined by a guided filter of the photo.  Returns
    (done, skipped); a photo without landmarks, without an edit or (with label_dir) without a label map is reported and left out.
    png='device': .png names are encoded on the device (the photo-sized result is never downloaded).  jpeg='device': the same for
    .jpg / .jpeg names, to the bytes Pillow writes at jpeg_quality and jpeg_subsampling (0 / '444' or 2 / '420'); jpeg='host' passes
    those two to Pillow when they are not its defaults.  decode='device': the photos and the edits are decoded on the device, as in
    crop_faces (stats['fallbacks']: the files Pillow decoded after all).
    orient, landmark_frame: as in crop_faces -- the PHOTO is made upright before the plan is made and the result is the upright,
    photo-sized picture; edits and label maps are the crop job's own outputs and are taken as they are.  metadata='keep': the result
    carries the photo's ICC profile and its EXIF block, with orient without the orientation tag (the pixels are upright now), without
    orient with it (they are still the stored ones); 'drop' (default): neither path carries EXIF or ICC data over, as before."""
    from PIL import Image
    from .alignment import align_plan
    if matte is not None and label_dir is None:
        raise ValueError('matte refines a weight map: it needs label_dir')
    _check_photo_options(orient, landmark_frame, metadata)
    keep = metadata == 'keep'
    os.makedirs(out_dir, exist_ok=True)
    encoder = _png_encoder(png, aligner)
    jpeg_encoder, jpeg_options = _jpeg_writer(jpeg, jpeg_quality, jpeg_subsampling, aligner)
    reader = _photo_reader(decode, aligner)
    read = read_rgb if reader is None else reader.read_rgb
    done, skipped = [], []
    for n in shard(list_images(photo_dir), rank, world):
        lm = find_landmarks(landmarks, dataset, n)
        if lm is None or not os.path.exists(os.path.join(edit_dir, n)):
            print(f'uncrop: no {"landmarks" if lm is None else "edit"} for {n}, skipped')
            skipped.append(n)
            continue
        label = None if label_dir is None else os.path.join(label_dir, os.path.splitext(n)[0] + '.png')
        if label is not None and not os.path.exists(label):
            print(f'uncrop: no label map for {n}, skipped')
            skipped.append(n)
            continue
        (photo, meta), edit = _read_photo(reader, os.path.join(photo_dir, n), orient, keep), read(os.path.join(edit_dir, n))
        lm = _photo_landmarks(lm, meta, photo.shape, orient, landmark_frame)
        kept = _kept_metadata(meta, keep, n)
        lists = {k: [v] for k, v in kept.items()}
        S = int(edit.shape[0]) if size is None else int(size)
        if edit.shape[:2] != (S, S):
            raise ValueError(f'{os.path.join(edit_dir, n)}: expected a {S} x {S} crop, got {edit.shape[1]} x {edit.shape[0]}')
        plan = align_plan(lm[:68], photo.shape[0], photo.shape[1], S)
        if label is None:
            out = aligner.paste_back(photo, edit, plan)[0]
        else:
            out = aligner.paste_back(photo, edit, plan, weight=label_weight(label, S), matte=matte)[0]
        if encoder is not None and _is_png(n):
            encoder.write([os.path.join(out_dir, n)], out[None], **lists)
        elif jpeg_encoder is not None and _is_jpeg(n):
            jpeg_encoder.write([os.path.join(out_dir, n)], out[None], **jpeg_options, **lists)
        else:
            Image.fromarray(out.cpu().numpy()).save(os.path.join(out_dir, n), **(jpeg_options if _is_jpeg(n) else {}), **kept)
        done.append(n)
    if stats is not None:
        stats['fallbacks'] = 0 if reader is None else reader.fallbacks
    return done, skipped


def pool_candidates(root: str, datasets: Sequence[str] = None) -> List[tuple]:
    """(dataset, label file name) of every label PNG under <root>/<dataset>/label, sorted; datasets: default every
    sub-directory of root that has a label folder."""
    if datasets is None:
        datasets = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d, 'label')))
    return [(d, n) for d in datasets for n in list_images(os.path.join(root, d, 'label'))]


def random_pairs(candidates: Sequence[tuple], n: int, seed: int) -> List[tuple]:
    """n (hair, face) pairs drawn with replacement from the candidates, a function of (candidates, n, seed) alone -- every rank
    draws the same list and takes its shard (the reference seeds each thread with the time)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(candidates), size=(n, 2)) if len(candidates) else np.zeros((0, 2), np.int64)
    return [(candidates[int(i)], candidates[int(j)]) for i, j in idx]


def read_pairs_file(path: str) -> List[tuple]:
    """Lines `hair_dataset hair_name face_dataset face_name` (blank lines and lines starting with # are skipped)."""
    pairs = []
    with open(path) as f:
        for k, line in enumerate(f, 1):
            w = line.split()
            if not w or w[0].startswith('#'):
                continue
            if len(w) != 4:
                raise ValueError(f'{path}:{k}: expected `hair_dataset hair_name face_dataset face_name`, got {line.strip()!r}')
            pairs.append(((w[0], w[1]), (w[2], w[3])))
    return pairs


def pool_name(hair: tuple, face: tuple, rank: int) -> str:
    """adaptor_generation.py:33-36: the numbers are the last five characters of the file names without their extension."""
    num = lambda n: os.path.splitext(n)[0][-5:]
    return '%s___%s___%s___%s___%02d.png' % (hair[0], num(hair[1]), face[0], num(face[1]), rank)


def warp_pool(warper, root: str, pool_dir: str, landmarks: Dict[str, np.ndarray], pairs: Sequence[tuple], batch: int = 16,
              rank: int = 0, world: int = 1, only_hair: bool = False):
    """The adaptor warp pool (adaptor_generation.py:31-52) for this rank's shard of `pairs` = [((hair_dataset, hair_name),
    (face_dataset, face_name)), ...]: the hair of <root>/<hair_dataset>/label/<hair_name> warped onto the face parsing, `batch`
    pairs per warper.warp_batch(mesher='device') call (`warper`: warping.MaskWarper; landmarks: name -> [81,2] in [0,1], looked up
    like the crop job's).  Writes <pool_dir>/<pool_name>: the label map, or (label == 13) * 255 with only_hair.
    Returns (done, skipped): the files written, and the 'dataset/name' entries without landmarks (reported, their pairs left
    out) plus the pairs whose points the device mesher refused."""
    os.makedirs(pool_dir, exist_ok=True)
    done, skipped, ready = [], [], []
    for hair, face in shard(list(pairs), rank, world):
        lms = [find_landmarks(landmarks, d, n) for d, n in (hair, face)]
        for (d, n), lm in zip((hair, face), lms):
            if lm is None and f'{d}/{n}' not in skipped:
                print(f'warp-pool: no landmarks for {d}/{n}, skipped')
                skipped.append(f'{d}/{n}')
        if lms[0] is not None and lms[1] is not None:
            ready.append((hair, face, np.asarray(lms[0], np.float64)[:81], np.asarray(lms[1], np.float64)[:81]))
    label = lambda e: read_gray(os.path.join(root, e[0], 'label', e[1]))
    for group in batches(ready, batch):
        out = warper.warp_batch(np.stack([label(g[0]) for g in group]), np.stack([label(g[1]) for g in group]),
                                np.stack([g[2] for g in group]), np.stack([g[3] for g in group]), mesher='device')
        out = out.cpu().numpy() if hasattr(out, 'cpu') else np.asarray(out)
        status = getattr(warper, 'last_mesh_status', None)
        status = np.zeros(len(group), np.int64) if status is None else np.asarray(status.cpu() if hasattr(status, 'cpu') else status)
        for g, lab, st in zip(group, out, status):
            name = pool_name(g[0], g[1], rank)
            if int(st) != 0:
                print(f'warp-pool: the mesher refused {name} (status {int(st)}), skipped')
                skipped.append(name)
                continue
            write_label_png(os.path.join(pool_dir, name), (lab == 13) * 255 if only_hair else lab)
            done.append(name)
    return done, skipped


def _main_warp_pool(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset warp-pool', description='Warp hair masks onto faces for many hair / face pairs')
    ap.add_argument('root', help='directory with <dataset>/label/<name>.png, as the masks job writes them')
    ap.add_argument('pool_dir', help='directory for the warped label maps')
    ap.add_argument('--landmarks', required=True, help='.npz or pickled dict: image name -> [81,2] landmarks in [0,1]')
    ap.add_argument('--pairs', type=int, default=None, help='number of random hair / face pairs (with --seed)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--pairs-file', default=None, help='lines `hair_dataset hair_name face_dataset face_name`')
    ap.add_argument('--datasets', nargs='*', default=None, help='datasets to draw from (default: every one under root)')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--only-hair', action='store_true', help='write (label == 13) * 255 instead of the label map')
    args = ap.parse_args(argv)
    if (args.pairs is None) == (args.pairs_file is None):
        ap.error('give either --pairs N or --pairs-file FILE')
    import torch
    from . import lib
    from .warping import MaskWarper
    rank, world, local = _dist_env()
    torch.cuda.set_device(local)
    landmarks = load_landmarks(args.landmarks)
    if args.pairs_file is not None:
        pairs = read_pairs_file(args.pairs_file)
    else:
        cands = pool_candidates(args.root, args.datasets)
        have = [c for c in cands if find_landmarks(landmarks, c[0], c[1]) is not None]
        for d, n in sorted(set(cands) - set(have)):
            print(f'warp-pool: no landmarks for {d}/{n}, not drawn')
        pairs = random_pairs(have, args.pairs, args.seed)
    warper = MaskWarper(lib.Handle(local), torch.device('cuda', local))
    done, skipped = warp_pool(warper, args.root, args.pool_dir, landmarks, pairs, args.batch, rank, world, args.only_hair)
    print(f'rank {rank}/{world}: {len(done)} files, {len(skipped)} skipped')


def load_search_images(img_dir: str, size: int, count: int, list_file: str = None) -> np.ndarray:
    """The images of a direction search: the first `count` of the sorted directory (or of the names in `list_file`, one per line), each
    as HairEditor.preprocess_img makes it: cv2-bilinear resize to size x size, / 127.5 - 1, float32 [I,3,size,size]."""
    from . import hostutil as U
    if list_file is not None:
        with open(list_file) as f:
            names = [ln.strip() for ln in f if ln.strip() and not ln.startswith('#')]
    else:
        names = list_images(img_dir)
    names = names[:count]
    if not names:
        raise ValueError(f'{img_dir}: no images to search on')
    imgs = [U.resize_bilinear(read_rgb(os.path.join(img_dir, n)).astype('uint8'), (size, size)) for n in names]
    return np.stack([(np.transpose(im, [2, 0, 1]) / 127.5 - 1.0).astype(np.float32) for im in imgs])


def _main_directions(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset directions', description='Search editing directions of the shape / texture latent')
    ap.add_argument('img_dir')
    ap.add_argument('--att', choices=('shape', 'texture'), required=True)
    ap.add_argument('--weights', default='procedural', help="'procedural' or the root of the reference's checkpoint tree")
    ap.add_argument('--used-dir', default=None, help='folder of the direction pickles already in use (*_dir_used)')
    ap.add_argument('--out', default='direction_find')
    ap.add_argument('--n', type=int, default=300, help='candidates')
    ap.add_argument('--images', type=int, default=10)
    ap.add_argument('--values', type=int, default=6, help='slider values per image, linspace(-max_val, max_val)')
    ap.add_argument('--max-val', type=float, default=2.5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--noise-seed', type=int, default=0)
    ap.add_argument('--size', type=int, default=256, choices=(256, 512))
    ap.add_argument('--cell', type=int, default=None, help='side of a sheet cell in pixels (default: the image size)')
    ap.add_argument('--sheets', default='all', help='all | top:K | none.  top:K scores every candidate first, then sweeps the K best of EACH rank a second time into sheets: '
                                                     'W ranks write up to W * K sheets')
    ap.add_argument('--list', default=None, help='file with the image names to use, one per line')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--png', choices=('host', 'device'), default='host', help='who writes PNG files: Pillow on the host (default) or ch_png_encode on the device (same pixels, other file bytes)')
    ap.add_argument('--png-stride', action='store_true', help='with --png device: also match at the sheet\'s column pitch, (cell + margin) * 3 bytes, where the columns of a row '
                                                              'repeat each other (ch_png_encode_dist): same pixels, smaller files.  Off by default')
    args = ap.parse_args(argv)
    if args.png_stride and args.png != 'device':
        ap.error('--png-stride needs --png device')
    import torch
    from . import directions as DS
    from .pipeline import EditPipeline
    DS.parse_sheets(args.sheets)
    rank, world, local = _dist_env()
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)      # only a barrier before the merge
    torch.cuda.set_device(local)
    weights = None
    if args.weights != 'procedural':
        from .checkpoints import reference_checkpoints
        weights = reference_checkpoints(args.weights)
    pipe = EditPipeline(weights, device=local, img_size=args.size, max_batch=args.batch)
    imgs = torch.from_numpy(load_search_images(args.img_dir, args.size, args.images, args.list))
    search = DS.DirectionSearch(pipe, imgs, noise_seed=args.noise_seed)
    recs = DS.find_directions(search, args.att, DS.load_used(args.used_dir), args.out, n=args.n,
                              values=np.linspace(-args.max_val, args.max_val, args.values), seed=args.seed, rank=rank, world=world,
                              sheets=args.sheets, cell=args.cell, png=args.png, png_stride=args.png_stride)
    if dist is not None:
        dist.barrier()
    if rank == 0:
        DS.merge_scores(args.out, world)
    print(f'rank {rank}/{world}: {len(recs)} candidates')
    if dist is not None:
        dist.destroy_process_group()


def _main_use_direction(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset use-direction', description='Copy a found direction into the used set')
    ap.add_argument('out', help='the --out folder of the directions job')
    ap.add_argument('att', choices=('shape', 'texture'))
    ap.add_argument('index', type=int)
    ap.add_argument('used_dir')
    args = ap.parse_args(argv)
    from .directions import use_direction
    print(use_direction(args.out, args.att, args.index, args.used_dir))


def _dist_env():
    return int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('LOCAL_RANK', '0'))


def main(argv=None):
    import argparse
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == 'crop':
        return _main_crop(argv[1:])
    if argv and argv[0] == 'uncrop':
        return _main_uncrop(argv[1:])
    if argv and argv[0] == 'warp-pool':
        return _main_warp_pool(argv[1:])
    if argv and argv[0] == 'median':
        return _main_median(argv[1:])
    if argv and argv[0] == 'directions':
        return _main_directions(argv[1:])
    if argv and argv[0] == 'use-direction':
        return _main_use_direction(argv[1:])
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('job', choices=('masks', 'codes') + tuple(COLOR_JOBS))
    ap.add_argument('root')
    ap.add_argument('dataset')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--img-size', type=int, default=256)
    ap.add_argument('--weights', default='reference', help="'reference' (the Google-Drive checkpoints under the reference's "
                                                           "paths) or 'procedural'")
    ap.add_argument('--png', choices=('host', 'device'), default='host', help='who writes PNG files: Pillow on the host (default) or ch_png_encode on the device (same pixels, other file bytes)')
    ap.add_argument('--decode', choices=('host', 'device'), default='host',
                    help='who decodes the files read: Pillow on the host (default) or the device.  rgb / colorvar: ch_png_decode (same pixels, same pickles).  '
                         'masks / codes: ch_jpeg_decode for .jpg / .jpeg, ch_png_decode for .png, then the resize and the normalisation there too '
                         '(ch_ingest_images: the same network input bit for bit); whatever the device does not take is Pillow\'s, file by file')
    args = ap.parse_args(argv)
    import torch
    from .hair_editor import HairEditor
    rank, world, local = _dist_env()
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)      # only a barrier before the merge
    torch.cuda.set_device(local)
    base = os.path.join(args.root, args.dataset)
    if args.job in COLOR_JOBS:           # no network weights: the colour statistics need only the library
        from . import lib
        from .colorstats import HairColorStats
        stats = HairColorStats(lib.Handle(local), torch.device('cuda', local))
        res = hair_color_stats(stats, os.path.join(base, 'images_256'), os.path.join(base, 'label'), args.root, args.dataset,
                               (args.job,), args.batch, rank, world, decode=args.decode)
        if dist is not None:
            dist.barrier()
        if rank == 0:
            merge_color_stats(args.root, (args.job,))
        print(f'rank {rank}/{world}: {len(res[args.job])} files')
        if dist is not None:
            dist.destroy_process_group()
        return
    he = HairEditor(True, True, weights=args.weights, device=local, img_size=args.img_size, max_batch=args.batch)
    stats = {}
    if args.job == 'masks':
        n = len(extract_masks(he, os.path.join(base, 'images_256'), os.path.join(base, 'label'), args.batch, rank, world, png=args.png,
                              decode=args.decode, stats=stats))
    else:
        code_dir = os.path.join(args.root, 'hair_info_all_dataset', 'sean_code')
        n = len(encode_sean_codes(he, os.path.join(base, 'images_256'), os.path.join(base, 'label'), code_dir, args.dataset,
                                  args.batch, rank, world, decode=args.decode, stats=stats))
        if dist is not None:
            dist.barrier()
        if rank == 0:
            merge_pickle_dir_to_dict(code_dir, os.path.join(args.root, 'sean_code_dict.pkl'))
    print(f'rank {rank}/{world}: {n} files' + (f', {stats["fallbacks"]} decoded by Pillow' if args.decode == 'device' else ''))
    if dist is not None:
        dist.destroy_process_group()


def _main_crop(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset crop', description='FFHQ-align a directory of photos from 68 landmarks')
    ap.add_argument('src_dir')
    ap.add_argument('root')
    ap.add_argument('dataset')
    ap.add_argument('--landmarks', required=True, help='.npz or pickled dict: image name -> [68,2] pixel landmarks')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--png', choices=('host', 'device'), default='host', help='who writes PNG files: Pillow on the host (default) or ch_png_encode on the device (same pixels, other file bytes)')
    ap.add_argument('--jpeg', choices=('host', 'device'), default='host', help='who writes .jpg / .jpeg files: Pillow on the host (default) or ch_jpeg_encode on the device (the same file bytes)')
    ap.add_argument('--jpeg-quality', type=int, default=75, help="JPEG quality 1..100 (default 75, Pillow's own default)")
    ap.add_argument('--jpeg-subsampling', choices=('420', '444'), default='420', help="JPEG chroma subsampling (default 420, Pillow's own default)")
    ap.add_argument('--decode', choices=('host', 'device'), default='host', help='who decodes the files read: Pillow on the host (default), or the device: ch_jpeg_decode for .jpg / .jpeg, ch_png_decode for .png (the same pixels, so the same results; whatever the device does not take is Pillow\'s, file by file)')
    ap.add_argument('--orient', action='store_true', help='make every photo upright by its EXIF orientation before it is used, as a viewer shows it (ch_orient_u8 with --decode device, Pillow\'s exif_transpose else; the same pixels)')
    ap.add_argument('--landmark-frame', choices=('upright', 'stored'), default='upright', help='with --orient: the landmarks are pixels of the upright photo (default) or of the stored one')
    ap.add_argument('--metadata', choices=('drop', 'keep'), default='drop', help="keep: write the photo's ICC profile and EXIF block (with --orient without its orientation tag) into the output; drop (default): neither")
    args = ap.parse_args(argv)
    if not 1 <= args.jpeg_quality <= 100:
        ap.error('--jpeg-quality must be in 1..100')
    import torch
    from . import lib
    from .alignment import FaceAligner
    rank, world, local = _dist_env()
    torch.cuda.set_device(local)
    aligner = FaceAligner(lib.Handle(local), torch.device('cuda', local))
    done, skipped = crop_faces(aligner, args.src_dir, os.path.join(args.root, args.dataset, 'images_256'), args.dataset,
                               load_landmarks(args.landmarks), args.size, rank, world, png=args.png, jpeg=args.jpeg,
                               jpeg_quality=args.jpeg_quality, jpeg_subsampling=args.jpeg_subsampling, decode=args.decode,
                               orient=args.orient, landmark_frame=args.landmark_frame, metadata=args.metadata)
    print(f'rank {rank}/{world}: {len(done)} files, {len(skipped)} without landmarks')


def _main_uncrop(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset uncrop', description='Paste edited FFHQ-aligned crops back into their photos')
    ap.add_argument('photos', help='directory of the original photos')
    ap.add_argument('edits', help='directory of the edited crops, one per photo, same file names')
    ap.add_argument('out', help='directory for the photo-sized results')
    ap.add_argument('--landmarks', required=True, help='.npz or pickled dict: image name -> [68,2] pixel landmarks (the crop job\'s file)')
    ap.add_argument('--size', type=int, default=None, help="the crops' side (default: each edit's own)")
    ap.add_argument('--dataset', default='', help="dataset name of '<dataset>___<name>' landmark keys")
    ap.add_argument('--labels', default=None, help='directory of 8-bit label PNGs of the crops (<stem>.png): paste only their hair')
    ap.add_argument('--matte', action='store_true', help='refine the hair region with a guided filter of the photo (needs --labels)')
    ap.add_argument('--matte-radius', type=int, default=None, help='matte window radius in photo pixels, 1..64 (default: 4 crop pixels)')
    ap.add_argument('--matte-eps', type=float, default=None, help='matte regularisation (default 1e-4)')
    ap.add_argument('--png', choices=('host', 'device'), default='host', help='who writes PNG files: Pillow on the host (default) or ch_png_encode on the device (same pixels, other file bytes)')
    ap.add_argument('--jpeg', choices=('host', 'device'), default='host', help='who writes .jpg / .jpeg files: Pillow on the host (default) or ch_jpeg_encode on the device (the same file bytes)')
    ap.add_argument('--jpeg-quality', type=int, default=75, help="JPEG quality 1..100 (default 75, Pillow's own default)")
    ap.add_argument('--jpeg-subsampling', choices=('420', '444'), default='420', help="JPEG chroma subsampling (default 420, Pillow's own default)")
    ap.add_argument('--decode', choices=('host', 'device'), default='host', help='who decodes the files read: Pillow on the host (default), or the device: ch_jpeg_decode for .jpg / .jpeg, ch_png_decode for .png (the same pixels, so the same results; whatever the device does not take is Pillow\'s, file by file)')
    ap.add_argument('--orient', action='store_true', help='make every photo upright by its EXIF orientation before it is used, as a viewer shows it (ch_orient_u8 with --decode device, Pillow\'s exif_transpose else; the same pixels)')
    ap.add_argument('--landmark-frame', choices=('upright', 'stored'), default='upright', help='with --orient: the landmarks are pixels of the upright photo (default) or of the stored one')
    ap.add_argument('--metadata', choices=('drop', 'keep'), default='drop', help="keep: write the photo's ICC profile and EXIF block (with --orient without its orientation tag) into the output; drop (default): neither")
    args = ap.parse_args(argv)
    if not 1 <= args.jpeg_quality <= 100:
        ap.error('--jpeg-quality must be in 1..100')
    matte = None
    if args.matte or args.matte_radius is not None or args.matte_eps is not None:
        if args.labels is None:
            ap.error('--matte, --matte-radius and --matte-eps need --labels DIR (the matte refines a per-image weight)')
        matte = {k: v for k, v in (('radius', args.matte_radius), ('eps', args.matte_eps)) if v is not None}
        from .alignment import matte_params
        try:
            matte_params(matte, 1.0)
        except ValueError as e:
            ap.error(str(e))
    import torch
    from . import lib
    from .alignment import FaceAligner
    rank, world, local = _dist_env()
    torch.cuda.set_device(local)
    aligner = FaceAligner(lib.Handle(local), torch.device('cuda', local))
    done, skipped = uncrop_faces(aligner, args.photos, args.edits, args.out, args.dataset, load_landmarks(args.landmarks), args.size,
                                 rank, world, label_dir=args.labels, matte=matte, png=args.png, jpeg=args.jpeg,
                                 jpeg_quality=args.jpeg_quality, jpeg_subsampling=args.jpeg_subsampling, decode=args.decode,
                                 orient=args.orient, landmark_frame=args.landmark_frame, metadata=args.metadata)
    print(f'rank {rank}/{world}: {len(done)} files, {len(skipped)} skipped')


def median_codes(medoid, root: str, out: str = None, tree: str = None) -> dict:
    """sean_codes/get_mean_code.py over <root>/sean_code_dict.pkl (what the codes job merges): per region the medoid and the mean of
    the codes of the images that have the region (`medoid`: stylestats.StyleMedoid).  Writes `out` (default
    <root>/mean_style_code.npz, the packaged file's format) and, with `tree`, the reference's <tree>/mean_style_code/{mean,median}/<i>/
    ACE.npy layout; prints count and chosen key per region.  Single process: no rank sharding at this cost."""
    from . import stylestats as SS
    with open(os.path.join(root, 'sean_code_dict.pkl'), 'rb') as f:
        codes = pickle.load(f)
    if not isinstance(codes, dict) or not codes:
        raise ValueError(f'{root}/sean_code_dict.pkl: expected a non-empty dict of key -> [19,512] style codes')
    res = medoid.median_style_codes(codes)
    SS.save_mean_style_code(out if out is not None else os.path.join(root, 'mean_style_code.npz'), res)
    if tree is not None:
        SS.write_reference_tree(tree, res)
    for j in range(SS.N_REGIONS):
        chosen = res['keys'][res['index'][j]] if res['index'][j] >= 0 else '(no image has it: packaged row kept)'
        print(f'region {j:2d}: {int(res["count"][j]):6d} codes  median = {chosen}')
    return res


def _main_median(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='ctrlhair_amd.dataset median', description='Per-region median (medoid) and mean style codes')
    ap.add_argument('root')
    ap.add_argument('--out', default=None, help='.npz to write (default <root>/mean_style_code.npz)')
    ap.add_argument('--tree', default=None, help="also write the reference's mean_style_code/{mean,median}/<i>/ACE.npy tree here")
    args = ap.parse_args(argv)
    import torch
    from . import lib
    from .stylestats import StyleMedoid
    _, _, local = _dist_env()
    torch.cuda.set_device(local)
    return median_codes(StyleMedoid(lib.Handle(local), torch.device('cuda', local)), args.root, args.out, args.tree)


if __name__ == '__main__':
    main()
