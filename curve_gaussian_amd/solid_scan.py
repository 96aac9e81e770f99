"""``python -m curve_gaussian_amd.solid_scan <shape> <out_dir>``: write a solid synthetic scan (scene/solid_scan.py)."""
import sys

from .scene.solid_scan import main

if __name__ == "__main__":
    sys.exit(main())
