"""Writes tests/golden/jpeg_index_cases.npz: PIL-written quality-100 noise files, 64 x 80, for the two POSITION cases of
the JPEG index (include/fastvim_hip.h at THE INDEX) that tests/test_jpeg_index_cpu.py asserts are present among their
groups of one MCU:

  A  a group whose first bit follows a stuffed 0xFF 0x00 pair with bit offset 0: the entry's byte is the one behind the
     stuffed 0x00;
  B  a group that starts inside a byte (bit offset 1..7) whose predecessor in the stream is a data 0xFF: the two file bytes
     in front of the entry's byte are 0xFF 0x00.

Quality-100 noise makes long codes and many 0xFF bytes, but a data 0xFF right in front of an MCU border is rare -- the
eight bits that end an MCU have to be ones: B shows about once in 5 000 borders, A about once in twenty million (three files among the first
263 000 seeds, all of them grayscale).  ``--search`` goes
through the seeds with the library's own builder and prints the first (seed, class) files that show each case; FILES
lists the ones picked (the test checks the cases on the restatement's index).  Run where PIL (with libjpeg-turbo) is:
``python tests/golden/gen_jpeg_index.py``."""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("444", "422", "420", "gray")
H, W = 64, 80
FILES = ((96, "422"), (99, "444"), (106096, "gray"))          # (seed, sampling class): B, B and A of --search


def one(seed, cls):
    k = CLASSES.index(cls)
    a = np.random.default_rng(1000 * seed + k).integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = io.BytesIO()
    if cls == "gray":
        Image.fromarray(a).convert("L").save(b, "JPEG", quality=100)
    else:
        Image.fromarray(a).save(b, "JPEG", quality=100, subsampling=k)
    return b.getvalue()


def position_cases(raw, index):
    """(groups of case A, groups of case B) of an index of ``raw``."""
    e = np.frombuffer(index, "<u4")[6592 // 4:].reshape(-1, 4)[:-1]
    a = [g for g, (byte, bit) in enumerate(e[:, :2]) if raw[byte - 2:byte] == b"\xff\x00" and bit == 0]
    b = [g for g, (byte, bit) in enumerate(e[:, :2]) if raw[byte - 2:byte] == b"\xff\x00" and bit > 0]
    return a, b


def search(limit=400000, want=2):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from fastvim_amd import jpeg
    found = ([], [])
    for seed in range(limit):
        for cls in CLASSES:
            raw = one(seed, cls)
            for case, groups in zip(found, position_cases(raw, jpeg.build_index(raw, 1))):
                if groups and len(case) < want:
                    case.append((seed, cls, groups))
        if all(len(case) >= want for case in found):
            break
    return found


def main():
    assert features.check_feature("libjpeg_turbo"), "the fixtures are libjpeg-turbo's output"
    if "--search" in sys.argv:
        for name, case in zip("AB", search()):
            print("case", name, case)
        return
    data = {"pil_version": np.array(PIL.__version__), "jpeg_version": np.array(str(features.version("jpg")))}
    names = []
    for seed, cls in FILES:
        raw = one(seed, cls)
        name = f"{H}x{W}_{cls}_q100_noise_s{seed}"
        names.append(name)
        data["jpg_" + name] = np.frombuffer(raw, np.uint8)
        data["rgb_" + name] = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))
    data["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg_index_cases.npz")
    np.savez_compressed(path, **data)
    print(path, len(names), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
