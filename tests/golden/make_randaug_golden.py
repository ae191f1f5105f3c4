"""Writes tests/golden/randaug_cases.npz with Pillow: inputs and Pillow's outputs for every op kind of mvf_frames_randaug_u8 (RGB images; the BGR cases are
the same images with the channels reversed before and after Pillow).  Made with Pillow 12.2.0:

    python tests/golden/make_randaug_golden.py

pil_op is also what tests/test_randaug_cpu.py compares with directly where Pillow is installed."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "randaug_cases.npz")
FILL = (124, 116, 104)                    # RGB
FACTORS = (0.1, 0.55, 1.0, 1.45, 1.9)     # blends on both sides of 1


def pil_op(rgb, name, arg, fill=FILL):
    """Pillow's (timm's) op `name` on an RGB uint8 image (h, w, 3); `arg` as mvfnet_amd.randaug.op_row takes it."""
    from PIL import Image, ImageEnhance, ImageOps
    img = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
    w, h = img.size
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    kw = dict(resample=Image.BILINEAR, fillcolor=tuple(fill))
    if name == "Identity":
        out = img
    elif name == "Invert":
        out = ImageOps.invert(img)
    elif name == "AutoContrast":
        out = ImageOps.autocontrast(img)
    elif name == "Equalize":
        out = ImageOps.equalize(img)
    elif base == "Posterize":
        out = img if arg >= 8 else ImageOps.posterize(img, int(arg))
    elif base == "Solarize":
        out = ImageOps.solarize(img, int(arg))
    elif name == "SolarizeAdd":
        out = img.point([min(255, i + int(arg)) if i < 128 else i for i in range(256)] * 3)
    elif base in ("Color", "Contrast", "Brightness", "Sharpness"):
        out = getattr(ImageEnhance, base)(img).enhance(arg)
    elif name == "Rotate":
        out = img.rotate(arg, **kw)
    elif name == "ShearX":
        out = img.transform(img.size, Image.AFFINE, (1, arg, 0, 0, 1, 0), **kw)
    elif name == "ShearY":
        out = img.transform(img.size, Image.AFFINE, (1, 0, 0, arg, 1, 0), **kw)
    elif name == "TranslateXRel":
        out = img.transform(img.size, Image.AFFINE, (1, 0, arg * w, 0, 1, 0), **kw)
    elif name == "TranslateYRel":
        out = img.transform(img.size, Image.AFFINE, (1, 0, 0, 0, 1, arg * h), **kw)
    else:
        raise ValueError(name)
    return np.asarray(out.convert("RGB"), dtype=np.uint8).copy()


def images():
    """Small inputs: a textured 37 x 53 image whose equalisation needs the 255 clamp, a 19 x 23 one, a 7 x 5 one with a constant channel, a narrow-range
    one, and the tiny sizes."""
    rng = np.random.RandomState(20240607)

    def textured(h, w):
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], -1)
        return np.clip(base + rng.randint(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)
    const = textured(7, 5)
    const[..., 1] = 77
    narrow = (100 + rng.randint(0, 23, size=(19, 23, 3))).astype(np.uint8)
    return [textured(37, 53), textured(19, 23), const, narrow, textured(3, 3), textured(2, 5), textured(1, 2), textured(1, 1)]


def cases():
    """(op name, argument, image index)."""
    c = [("Identity", 0, 1), ("Invert", 0, 1)]
    c += [("Posterize", b, 1) for b in (0, 2, 4, 7)] + [("PosterizeIncreasing", 3, 2)]
    c += [("Solarize", v, 1) for v in (0, 100, 256)] + [("SolarizeIncreasing", 77, 2)]
    c += [("SolarizeAdd", v, 1) for v in (0, 60, 110)]
    c += [("AutoContrast", 0, i) for i in (0, 1, 2, 3, 6, 7)] + [("Equalize", 0, i) for i in (0, 1, 2, 3, 4, 6, 7)]
    for name in ("Brightness", "Contrast", "Color", "Sharpness"):
        c += [(name, f, 1) for f in FACTORS] + [(name + "Increasing", f, 0) for f in (0.37, 1.63)] + [(name, 1.3, i) for i in (2, 4, 5, 7)]
    c += [("Rotate", d, 0) for d in (21.0, -30.0, 7.5)] + [("ShearX", 0.21, 0), ("ShearY", -0.3, 0), ("TranslateXRel", 0.315, 0), ("TranslateYRel", -0.45, 0)]
    c += [("Rotate", 13.0, 4), ("ShearX", 0.3, 5), ("TranslateXRel", 0.45, 6), ("Rotate", 30.0, 7)]
    return c


def main():
    import PIL
    imgs, cs = images(), cases()
    data = {"pillow_version": np.array(PIL.__version__), "fill": np.array(FILL, dtype=np.uint8),
            "names": np.array([n for n, _, _ in cs]), "args": np.array([float(a) for _, a, _ in cs], dtype=np.float64),
            "image": np.array([i for _, _, i in cs], dtype=np.int32)}
    for i, im in enumerate(imgs):
        data["img_%d" % i] = im
    for k, (name, arg, i) in enumerate(cs):
        data["out_%d" % k] = pil_op(imgs[i], name, arg)
    np.savez_compressed(OUT, **data)
    print("%s: %d cases, %d images, %d bytes" % (OUT, len(cs), len(imgs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
