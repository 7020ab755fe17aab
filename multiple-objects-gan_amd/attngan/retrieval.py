"""Host side of R-precision, the AttnGAN paper's text-image retrieval metric (the reference repository has
no code for it).

An image counts as retrieved when, among its own caption and `Rn` (99) captions of OTHER images, its own caption has the highest
cosine similarity of DAMSM image code and sentence code.  R-precision is the share of retrieved images, reported as mean +- std
over equal consecutive folds (ten folds of 3000 images in the paper's protocol).

  * `SentenceBank`   every caption of a split encoded once (the sentence codes stay on the device) + which image each belongs to;
  * `draw_mismatched` the (Q, Rn) table of bank rows a batch of queries is ranked against;
  * `fold_stats`     ranks -> r_precision, mean, std;
the ranking itself is one launch, hip/ops.retrieval_rank.  Nothing in this module's logic needs a GPU: the bank takes any callable
text encoder and builds on the device its parameters live on.
"""
import numpy as np
import torch

ENCODER_BATCH = 64          # captions per text-encoder call: the one-launch encoder's limit (csrc/mogan_rnn.hip, B <= 64)


def fit_caption(cap, words_num, rng):
    """datasets.TextDataset.get_caption's rule with the draw taken from `rng`: a caption of more than `words_num` tokens keeps a
    sorted random subset of `words_num` of them.  Returns the int64 tokens (at most words_num)."""
    cap = np.asarray(cap).astype('int64').reshape(-1)
    if len(cap) <= words_num:
        return cap
    return cap[np.sort(rng.permutation(len(cap))[:words_num])]


class SentenceBank:
    """bank (N, nef) fp32 on the device: row i = the sentence code of caption i; image_index (N,) host int64: the image caption i
    belongs to; key_to_image: the loader's sample key -> image number (None where the caller maps keys itself)."""

    def __init__(self, bank, image_index, key_to_image=None):
        self.bank, self.image_index, self.key_to_image = bank, np.asarray(image_index, dtype=np.int64), key_to_image
        assert self.bank.shape[0] == self.image_index.shape[0]

    def __len__(self):
        return int(self.bank.shape[0])

    def images_of(self, keys):
        return np.asarray([self.key_to_image[k] for k in keys], dtype=np.int64)

    @classmethod
    def build(cls, text_encoder, captions, image_index, words_num, seed, chunk=1024, key_to_image=None):
        """Encode every caption once, in eval mode and without gradients.  The long-caption subsets are drawn from the bank's own
        RandomState(seed), in caption order, before anything is grouped: the rows do not depend on `chunk`.  Each chunk of
        consecutive captions is sorted by falling length (the packed-sequence order the encoder expects), encoded ENCODER_BATCH at a
        time and scattered back to its rows."""
        rng = np.random.RandomState(seed)
        caps = [fit_caption(c, words_num, rng) for c in captions]
        N = len(caps)
        if N != len(image_index):
            raise ValueError("SentenceBank: %d captions, %d image numbers" % (N, len(image_index)))
        device = next(text_encoder.parameters()).device
        was = text_encoder.training
        text_encoder.eval()
        bank = None
        try:
            with torch.no_grad():
                for c0 in range(0, N, max(1, int(chunk))):
                    rows = np.arange(c0, min(N, c0 + max(1, int(chunk))))
                    lens = np.asarray([len(caps[i]) for i in rows])
                    rows = rows[np.argsort(-lens, kind="stable")]
                    for b0 in range(0, len(rows), ENCODER_BATCH):
                        sub = rows[b0:b0 + ENCODER_BATCH]
                        sl = [len(caps[i]) for i in sub]
                        tok = np.zeros((len(sub), words_num), dtype=np.int64)
                        for j, i in enumerate(sub):
                            tok[j, :sl[j]] = caps[i]
                        _, sent = text_encoder(torch.from_numpy(tok).to(device), torch.tensor(sl),
                                               text_encoder.init_hidden(len(sub)))
                        if bank is None:
                            bank = torch.empty((N, sent.shape[1]), dtype=torch.float32, device=device)
                        bank[torch.from_numpy(sub).to(device)] = sent.float()
        finally:
            text_encoder.train(was)
        return cls(bank, image_index, key_to_image)

    @classmethod
    def from_dataset(cls, text_encoder, dataset, words_num, seed, chunk=1024):
        captions, image_index, keys = dataset_captions(dataset)
        return cls.build(text_encoder, captions, image_index, words_num, seed, chunk,
                         key_to_image={k: i for i, k in enumerate(keys)})


def dataset_captions(dataset):
    """(captions, image_index, keys) of a split.  TextDataset: its `captions` list holds `embeddings_num` consecutive captions per
    entry of `filenames`.  Any other dataset of the same sample structure (SyntheticTextDataset): one caption per index, read
    through dataset[i] = (imgs, caps (T, 1), cap_len, class_id, key, ...)."""
    if hasattr(dataset, "captions") and hasattr(dataset, "filenames"):
        per = int(dataset.embeddings_num)
        n_img = len(dataset.filenames)
        captions = list(dataset.captions[:n_img * per])
        return captions, np.arange(len(captions), dtype=np.int64) // per, list(dataset.filenames)
    captions, keys = [], []
    for i in range(len(dataset)):
        sample = dataset[i]
        captions.append(np.asarray(sample[1]).reshape(-1)[:int(sample[2])])
        keys.append(sample[4])
    return captions, np.arange(len(captions), dtype=np.int64), keys


def _distinct(rng, M, k):
    """k distinct numbers of range(M) in drawing order.  A permutation costs O(M) per query -- 200 000 captions in a COCO split,
    30 000 queries --, so for k << M the numbers are drawn one batch at a time and repeats are dropped."""
    if 3 * k >= M:
        return rng.permutation(M)[:k].astype(np.int64)
    out, seen = [], set()
    while len(out) < k:
        for v in rng.randint(0, M, size=k - len(out) + 8).tolist():
            if v not in seen:
                seen.add(v)
                out.append(v)
                if len(out) == k:
                    break
    return np.asarray(out, dtype=np.int64)


def draw_mismatched(image_index, query_images, Rn, rng):
    """int32 (Q, Rn): per query `Rn` distinct bank rows, drawn without replacement by `rng` (a numpy RandomState) among the rows
    whose image is not the query's own.  ValueError when a query has fewer than Rn such rows."""
    image_index = np.asarray(image_index)
    N, Rn = len(image_index), int(Rn)
    out = np.empty((len(query_images), Rn), dtype=np.int32)
    for q, img in enumerate(query_images):
        own = np.flatnonzero(image_index == img)
        if N - len(own) < Rn:
            raise ValueError("draw_mismatched: image %d has %d captions of other images to draw from, %d asked for"
                             % (int(img), N - len(own), Rn))
        # draw among the first N - len(own) numbers, then step over the own rows (ascending): uniform over the eligible rows
        pick = _distinct(rng, N - len(own), Rn)
        for o in own:
            pick[pick >= o] += 1
        out[q] = pick
    return out


def eligible(image_index, Rn):
    """whether every image of the bank has at least Rn captions of other images"""
    image_index = np.asarray(image_index)
    if len(image_index) == 0:
        return False
    return len(image_index) - int(np.bincount(image_index - image_index.min()).max()) >= int(Rn)


def fold_stats(ranks, folds=10):
    """ranks (n,): per image the number of mismatched captions that beat its own (0 = retrieved).  r_precision is the share of
    zeros over all n; mean / std (population) are over `folds` equal consecutive folds of n // folds images -- the remainder
    counts for r_precision only."""
    hit = (np.asarray(ranks).reshape(-1) == 0).astype(np.float64)
    n, folds = int(hit.size), int(folds)
    per = n // folds if folds > 0 else 0
    if per > 0:
        f = hit[:per * folds].reshape(folds, per).mean(1)
        mean, std = float(f.mean()), float(f.std())
    else:
        mean, std = float("nan"), float("nan")
    return {"r_precision": float(hit.mean()) if n else float("nan"), "mean": mean, "std": std, "n": n, "folds": folds}
