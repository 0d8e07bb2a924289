"""Writes tests/golden/alac_textbook.json: the handmade Apple Lossless packets (tests/alac_cases.handmade) and what the model
(tests/alac_textbook.py) made of them when they were pinned."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_alac_textbook  # noqa: E402

with open(os.path.join(HERE, "alac_textbook.json"), "w") as f:
    json.dump(test_alac_textbook.pins_now(), f, indent=1)
    f.write("\n")
