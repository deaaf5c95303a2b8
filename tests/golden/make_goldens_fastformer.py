"""Golden-vector generator for block_type "fastformer" - runs ONLY where the reference checkout exists (imports the live reference through
oracle/ref_import.py, like make_goldens.py).

Writes data only:
  state_dict_schema_LJSpeech_fastformer.json   key -> [shape, dtype, is_parameter] of the reference model
  g18_fastformer_eval.npz                      eval forward of a ragged B = 3 batch (two utterances padded)
  g18_fastformer_train_nodrop.npz              train forward with dropout off + gradients in the G4 style (head 64 + sum / norm)
  g18_fastformer_infer.npz                     inference branch (no targets) with p / e / d_control
Weights: oracle.weights.closed_form_state_dict, except that the logit projections `to_q_attn_logits` / `to_k_attn_logits` are ONE tensor
per stack in the reference (tied across layers, fastformer.py FFTBlock.__init__): every layer's key of a tied tensor gets the value of
layer 0's key (tied_from_layer0), and the tests load the same values.
Re-run:  python tests/golden/make_goldens_fastformer.py
"""
import os
import re
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_goldens as G  # noqa: E402  (installs the reference, builds closed-form weights, writes fixtures)
from ctts_amd.synthetic import make_batch  # noqa: E402

_TIED = re.compile(r"^(.*\.layer_stack\.layers\.)(\d+)(\.0\.fn\.to_[qk]_attn_logits\.(weight|bias))$")


def tied_from_layer0(sd):
    """every layer's tied logit-projection key takes the value of layer 0's key (the reference holds ONE tensor per stack)"""
    out = dict(sd)
    for k in sd:
        m = _TIED.match(k)
        if m:
            out[k] = sd[f"{m.group(1)}0{m.group(3)}"]
    return out


def drop_taps(name):
    """the tests compare model outputs and gradients only: the intermediate activations run_case also records (tap.*) are left out,
    which keeps each fixture small"""
    path = os.path.join(OUT, name + ".npz")
    z = np.load(path)
    arrs = {k: z[k] for k in z.files if not k.startswith("tap.")}
    np.savez_compressed(path, **arrs)
    print("kept", path, f"{os.path.getsize(path) / 1024:.0f} KB")


def main():
    torch.manual_seed(0)
    model, cfgs = G.build("LJSpeech", "fastformer")      # writes the schema file, loads closed-form weights
    model.load_state_dict(tied_from_layer0(G.closed_form_state_dict(model.state_dict())))
    enc = model.encoder.layer_stack.layers
    assert enc[0][0].fn.to_q_attn_logits is enc[-1][0].fn.to_q_attn_logits
    batch = make_batch([16, 11, 6], 5, seed=1818)      # B = 3, two padded utterances; fixtures stay small
    G.run_case(model, batch, "eval", "g18_fastformer_eval")
    G.run_case(model, batch, "train", "g18_fastformer_train_nodrop", with_grads=True)
    inf = dict(batch)
    inf.update(mels=None, mel_lens=None, max_mel_len=None, p_targets=None, e_targets=None, d_targets=None)
    G.run_case(model, inf, "eval", "g18_fastformer_infer", extra_kwargs=dict(p_control=1.1, e_control=0.9, d_control=2.0))
    for name in ("g18_fastformer_eval", "g18_fastformer_train_nodrop", "g18_fastformer_infer"):
        drop_taps(name)


if __name__ == "__main__":
    main()
