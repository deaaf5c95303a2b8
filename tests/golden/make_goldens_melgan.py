"""Writes tests/golden/melgan_state_dict_schema.json: the state-dict keys of the MelGAN generator (descriptinc/melgan-neurips
mel2wav/modules.py Generator(80, 32, 3)) with their shapes, in state-dict order, from the stock-torch build of the module table in
tests/melgan_restate.py - the key set a released checkpoint carries (126 entries, 4,266,050 parameters).

    python tests/golden/make_goldens_melgan.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import melgan_restate as MR  # noqa: E402

if __name__ == "__main__":
    sd = MR.stock_generator().state_dict()
    schema = {"entries": len(sd), "parameters": sum(v.numel() for v in sd.values()), "keys": {k: list(v.shape) for k, v in sd.items()}}
    assert schema["entries"] == 126 and schema["parameters"] == 4266050, (schema["entries"], schema["parameters"])
    with open(os.path.join(HERE, "melgan_state_dict_schema.json"), "w") as f:
        json.dump(schema, f, indent=0)
        f.write("\n")
    print("wrote melgan_state_dict_schema.json:", schema["entries"], "entries,", schema["parameters"], "parameters")
