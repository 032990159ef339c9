"""Writes tests/golden/kl_update_bits.npz: the output bits of every entry point that forms a KL term (the cases of tests/klbits_cases.py), from
whatever library MFVI_LIB_PATH names (default: this tree's build).  The committed file was recorded from a library built from the sources of
the commit BEFORE the KL kernels were folded into one templated family, so tests/test_gpu_kl_bits.py holds the
folded kernels to the bits of the separate ones.  Needs the GPU; nothing else.

The file holds four arrays: `digest_names` / `digests` (sha256 of the raw bytes of an output array), `value_names` / `values` (a float64
scalar KL; klbits_cases.record says which of them are held bitwise).  It is written with fixed zip timestamps: two recordings of the same
bits are the same bytes.

usage: [MFVI_LIB_PATH=.../libmfvi_hip.so] python scripts/make_golden_klbits.py [--out tests/golden/kl_update_bits.npz]"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(digests, exact, close):
    values = {"exact/" + k: v for k, v in exact.items()}
    values.update({"close/" + k: v for k, v in close.items()})
    dn, vn = sorted(digests), sorted(values)
    return dict(digest_names=np.array(dn, dtype="S"), digests=np.array([np.frombuffer(digests[k], np.uint8) for k in dn]),
                value_names=np.array(vn, dtype="S"), values=np.array([values[k] for k in vn], np.float64))


def write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[name], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kl_update_bits.npz"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mfvi_dip_mia_amd as M
    import klbits_cases
    arrays = tables(*klbits_cases.record(M))
    write(a.out, arrays)
    print("%s: %d digests, %d values, library %s" % (a.out, len(arrays["digests"]), len(arrays["values"]), M._lib.LIB_PATH))


if __name__ == "__main__":
    main()
