"""Shared inputs of the collection tests (tests/test_collection_gpu.py, tests/test_collection_inputs.py;
DESIGN.md §18), built from the yardsticks alone."""
import numpy as np

import flagged_inputs as FI


def flag_sets():
    """({"QI", "QR"} -> 100 query rows, [integer, jittered, integer] images of 250, 250 and 200 rows): 128-D rows
    of flagged_inputs.mixed_sets, whose planted near copies lie in all three images."""
    M = FI.mixed_sets()
    return {"QI": M["QI"][:100], "QR": M["QR"][:100]}, [M["TI"][:250], M["TR"][250:500], M["TI"][500:]]


def sqrt_rows():
    """Integer 128-D rows by their squared distance to the zero row: A 8,000,001 and B 8,000,000 (one sqrtf),
    C 8,000,005 (the next), N 7,999,752 (nearer), and a far row (128 x 255^2)."""
    far = np.full(128, 255, np.float32)
    tails = {"A": (43, 8, 3, 2, 0), "B": (43, 8, 2, 2, 2), "C": (43, 8, 3, 2, 2), "N": (40, 8, 3, 2, 0)}
    rows = {}
    for name, tail in tails.items():
        rows[name] = far.copy()
        rows[name][123:] = tail
    return rows, far


# where the rows sit: image 0 has 1,100 rows = 18 train tiles, which the i8 schedule cuts at tiles 8 and 16 (rows
# 512 and 1024).  A lane of the i8 kernel holds the rows of one lane half (bit 2 of the row) of one split in one
# list.  Rows 5 (A, the larger d^2), 13 (B), 21 and 29 (N) are one lane's: a list of 3 must keep row 5 and drop
# row 13, where a ranking on d^2 would keep row 13.  Row 9 (B) is row 5's r + 4: the other lane half.  Row 600 (B)
# falls into another split.  Image 1 (70 rows) holds the smaller d^2 (B) at a lower row than any of image 0's.
SQRT_IMG0 = ((5, "A"), (9, "B"), (13, "B"), (21, "N"), (29, "N"), (600, "B"), (700, "C"))
SQRT_IMG1 = ((2, "B"), (60, "A"))
# (image, row) by (sqrtf, image, row), and what a ranking on (d^2, image, row) would give
SQRT_ORDER = [(0, 21), (0, 29), (0, 5), (0, 9), (0, 13), (0, 600), (1, 2), (1, 60), (0, 700)]
SQRT_ORDER_ON_D2 = [(0, 21), (0, 29), (0, 9), (0, 13), (0, 600), (1, 2), (0, 5), (1, 60), (0, 700)]


def sqrt_images():
    rows, far = sqrt_rows()
    img0, img1 = np.tile(far, (1100, 1)), np.tile(far, (70, 1))
    for row, n in SQRT_IMG0:
        img0[row] = rows[n]
    for row, n in SQRT_IMG1:
        img1[row] = rows[n]
    return img0, img1
