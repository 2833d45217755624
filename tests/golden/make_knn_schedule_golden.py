"""Writes tests/golden/knn_schedule.json: per case of tests/test_knn_schedule.py the sha256 of the tables
that tests/cpp/knn_schedule_driver.cpp prints, with n_blocks, the work-item count, the partials total
and the mode.

The committed file was written once, from the verbatim move of the schedule out of api.cpp's build_tables
into csrc/knn_schedule.h (one function, the discarded static pass included), so it pins the tables of the
code before the move.  Do not regenerate it from restructured code: a digest that changes there is an
error in the restructuring.

    python tests/golden/make_knn_schedule_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "knn_schedule.json")


def main():
    if not os.path.exists(OUT):  # the test module reads the file at import
        with open(OUT, "w") as f:
            f.write("{}\n")
    import test_knn_schedule as T

    with tempfile.TemporaryDirectory() as d:
        exe = T.build_driver(os.path.join(d, "knn_schedule_driver"))
        gold = {name: T.summary(T.run_driver(exe, name)) for name in sorted(T.CASES)}
    with open(OUT, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, len(gold), "cases")


if __name__ == "__main__":
    main()
