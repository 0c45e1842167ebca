"""Write an image dataset directory (the ``--data_dir`` format of the ResNet replicas,
docs/get_started.md) from a seed: ``train_images.npy`` / ``train_labels.npy``, a val
split a quarter of the size, and ``meta.json``.  Images are colour-coded by class
(class colour + zero-mean pixel noise), so the label can be recovered from the
mean pixel and a few training steps already move the validation accuracy.

  python tools/make_image_dataset.py --out /tmp/images --n 2048 --size 40 --classes 10 --seed 0
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kubeflow_controller_amd.models.imagenet import write_synthetic_dataset  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="directory to write (created if missing)")
    ap.add_argument("--n", type=int, default=1024, help="training images")
    ap.add_argument("--size", type=int, default=40, help="image height = width")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n_val", type=int, default=None, help="validation images (default: n / 4)")
    a = ap.parse_args(argv)
    write_synthetic_dataset(a.out, a.n, a.size, a.classes, a.seed, a.n_val)
    print(f"wrote {a.out}: {a.n} training images {a.size}x{a.size}, {a.classes} classes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
