"""Write the frozen tables of a PretrainedAttentionClassifier: emb.npy [V, C] and its position twin [T, C].

    python tools/make_embeddings.py --from <experiment dir>/warmstart/params_0.npz --out results/pretrained_seq/emb.npy
    python tools/make_embeddings.py --random 10000 70 192 --seed 0 --out results/pretrained_seq/emb.npy

--from reads an AttentionClassifier params_*.npz (the warm start writes one per chain under <experiment dir>/warmstart/; the run
of experiments/mclmc_seqmod_pretraining*_synthetic.yaml is the one at the pretrained model's shape) or sample_*.npz (the leaves TokenEmbedding_0.Embedding.embedding and
TokenEmbedding_0.PositionEmbedding.embedding; a stacked file with a leading sample axis takes --index).  --random draws both
tables as normal with std 1 / sqrt(C), nn.Embed's initialiser, for synthetic runs.  The position table goes where the model
will look for it: the --out path with every 'emb' replaced by 'pos_emb' (mile_amd.spec.pretrained_table_paths), so
emb_large.npy pairs with pos_emb_large.npy.  Prints one JSON line with both paths and shapes.
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np

from mile_amd.spec import pretrained_table_paths

EMB_KEY = 'TokenEmbedding_0.Embedding.embedding'
POS_KEY = 'TokenEmbedding_0.PositionEmbedding.embedding'


def from_params(path, index=0):
    with np.load(path) as z:
        found = {}
        for key in z.files:
            for want in (EMB_KEY, POS_KEY):
                if key == want or key.endswith('.' + want):
                    found[want] = np.asarray(z[key])
    missing = [k for k in (EMB_KEY, POS_KEY) if k not in found]
    if missing:
        raise SystemExit(f'{path}: no {" / ".join(missing)} leaf (an AttentionClassifier params_*.npz or sample_*.npz?)')
    emb, pos = found[EMB_KEY], found[POS_KEY]
    if emb.ndim == 3:
        emb, pos = emb[index], pos[index]
    return emb, pos


def random_tables(V, T, C, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, C)) / np.sqrt(C), rng.standard_normal((T, C)) / np.sqrt(C)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--from', dest='src', help='AttentionClassifier params_*.npz or sample_*.npz')
    src.add_argument('--random', nargs=3, type=int, metavar=('V', 'T', 'C'), help='synthetic tables')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--index', type=int, default=0, help='sample of a stacked file')
    ap.add_argument('--out', required=True, help="the token table's path (model.emb_path)")
    a = ap.parse_args(argv)
    emb, pos = from_params(a.src, a.index) if a.src else random_tables(*a.random, a.seed)
    emb_path, pos_path = pretrained_table_paths(a.out)
    for path, table in ((emb_path, emb), (pos_path, pos)):
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        np.save(path, np.ascontiguousarray(table, dtype=np.float32))
    print(json.dumps({'emb': emb_path, 'emb_shape': list(emb.shape), 'pos': pos_path, 'pos_shape': list(pos.shape)}))


if __name__ == '__main__':
    main()
