"""Makes tests/golden/overlay_palette.npz from matplotlib (run where matplotlib is installed; no test imports it):

    python tests/golden/make_overlay_golden.py [--print-package-data]

- tab20 (20, 3) and nipy_spectral (256, 3) uint8: the colormaps' own tables, a channel c as round(c * 255);
- palette_<n> (n, 3) uint8 for several n on both sides of 20: the colours models/model_utils.py::plot_segmentation
  picks for n segments -- cmap(i) of tab20 for n <= 20, cmap(x) of nipy_spectral for x in np.linspace(0, 1, n) above.
`--print-package-data` prints the two tables as the literals of weed_instance_segmentation_amd/_palette.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = (1, 2, 19, 20, 21, 22, 37, 100, 255, 256, 257, 1000)


def u8(rgba):
    return np.round(np.asarray(rgba, np.float64)[..., :3] * 255).astype(np.uint8)


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    tab20, spectral = plt.get_cmap("tab20"), plt.get_cmap("nipy_spectral")
    out = {"tab20": u8([tab20(i) for i in range(20)]), "nipy_spectral": u8([spectral(i) for i in range(256)]),
           "counts": np.asarray(COUNTS, np.int64), "matplotlib_version": np.asarray(matplotlib.__version__)}
    for n in COUNTS:
        if n <= 20:
            out[f"palette_{n}"] = u8([tab20(i) for i in range(max(n, 1))])
        else:
            out[f"palette_{n}"] = u8([spectral(x) for x in np.linspace(start=0, stop=1, num=n)])
    np.savez_compressed(os.path.join(HERE, "overlay_palette.npz"), **out)
    if "--print-package-data" in sys.argv:
        print("TAB20 = (" + ", ".join(str(tuple(int(v) for v in c)) for c in out["tab20"]) + ")")
        hexed = out["nipy_spectral"].tobytes().hex()
        print("NIPY_SPECTRAL_HEX = (\n" + "\n".join(f'    "{hexed[i:i + 96]}"' for i in range(0, len(hexed), 96)) + ")")


if __name__ == "__main__":
    main()
