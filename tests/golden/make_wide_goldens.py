"""Regenerates tests/golden/wide/*.npz: reference runs of shapes that need the decoder's wide operand layout
(spVIPESmodule(decoder_slots="wide" | "auto"): more batch-covariate categories than the narrow 16 / 32 K slots take).

    python tests/golden/make_wide_goldens.py

Same recipe and file format as make_goldens.py (whose run_case this reuses, unchanged); the fixtures live in a subdirectory
because the narrow golden tests glob tests/golden/*.npz and build default (narrow) modules.  Load one with Golden("wide/<name>").
Only data is committed -- no reference source travels.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import load_reference, run_case  # noqa: E402

CASES = [
    # name, kwargs: 25 / 10 latents (the defaults) need the wide layout from n_batch 6 on
    ("label_train_batch12", dict(B=(16, 16), G=(48, 40), H=16, n_s=25, n_p=10, mode="label", seed=21, n_batch=12)),
    ("label_eval_batch14", dict(B=(16, 16), G=(48, 40), H=16, n_s=25, n_p=10, mode="label", training=False, seed=22, n_batch=14)),   # at the mixture GEMM's 320 columns
    ("paired_train_batch20", dict(B=(16, 16), G=(40, 36), H=16, n_s=6, n_p=3, mode="paired", seed=23, n_batch=20)),   # only the private regressor is too narrow
    ("label_train_batch12_c1dims", dict(B=(16, 16), G=(40, 36), H=16, n_s=10, n_p=5, mode="label", seed=24, n_batch=12)),
]


def main():
    ref = load_reference()
    os.makedirs(os.path.join(HERE, "wide"), exist_ok=True)
    for name, kw in CASES:
        run_case(ref, "wide/" + name, **kw)


if __name__ == "__main__":
    main()
