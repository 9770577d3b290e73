"""Dataset wrappers of experiments/data/utils.py and the device-resident loader this build prefers.

``Dataset`` (utils.py:5-15) normalises every item with the MNIST statistics (0.1307, 0.3081) and reshapes it to
(16, 1, 28, 28); ``Dataset_labels`` (utils.py:17-28) pairs frames with their time index.  Both are host-side and feed
``torch.utils.data.DataLoader`` exactly like the reference's.

``ResidentLoader``: rotating MNIST is 360 x 16 x 784 floats = 18 MB -- nothing on a 288 GB device.  The normalised set is
uploaded once; an epoch is a device-side permutation and every minibatch one ``index_select`` on the current stream, so the
training step (a replayed HIP graph reading a static input buffer) never waits for a host copy.

``subsample_frames``: irregularly observed sequences out of regularly sampled ones -- every sequence keeps its own sorted subset
of the frames, and the kept indices are its observation times in units of ``dt`` (``--subsample_frames``).

``ragged_frames``: the same with a different NUMBER of kept frames per sequence, as a padded minibatch with its frame counts
(``--ragged_frames``).
"""
import torch
from torch.utils import data

MNIST_MEAN, MNIST_STD = 0.1307, 0.3081


def normalise(frames):
    return (frames - MNIST_MEAN) / MNIST_STD


def subsample_frames(X, keep, lead, generator):
    """X (N,T,...) -> (X[:, idx] (N,keep,...), idx (N,keep) int64): per sequence a sorted set of ``keep`` distinct frame indices that
    always holds 0 .. lead-1 (the frames the encoders read: 1 for a first-order model, the velocity encoder's ``frames`` for a
    second-order one, which takes them to be consecutive); the other keep - lead are drawn uniformly without replacement from
    lead .. T-1.  Drawn on X's device from ``generator`` alone (a torch.Generator of that device): the global generators are
    not touched.  The time grid of sequence n is dt * idx[n]."""
    N, T = X.shape[0], X.shape[1]
    keep, lead = int(keep), int(lead)
    if lead < 1 or keep <= lead or keep > T:
        raise ValueError('subsample_frames: keep=%d must lie in (lead, T] = (%d, %d]: the first %d frame(s) are always kept and at '
                         'least one later frame is drawn' % (keep, lead, T, lead))
    # the keep - lead smallest of T - lead uniform scores: a uniform subset; sorted, and behind the leading frames
    scores = torch.rand((N, T - lead), device=X.device, generator=generator)
    tail = scores.argsort(dim=1)[:, :keep - lead].sort(dim=1).values + lead
    head = torch.arange(lead, device=X.device).expand(N, lead)
    idx = torch.cat((head, tail), dim=1)
    return X[torch.arange(N, device=X.device)[:, None], idx], idx


def ragged_frames(X, kmin, kmax, lead, generator):
    """X (N,T,...) -> (Xpad (N,kmax,...), idx (N,kmax) int64, n_obs (N,) int32): sequences with different NUMBERS of observations,
    as a padded minibatch.  Sequence n keeps k_n frames, k_n uniform in kmin .. kmax: a sorted set of distinct indices that always
    holds 0 .. lead-1, drawn as in ``subsample_frames`` (the k_n - lead smallest of T - lead uniform scores).  Behind them the target frames are zeros and the indices go on as idx[k_n-1] + 1, + 2, ...: they are times only --
    the padding keeps every row strictly increasing (an adaptive solver refuses a row that is not) and may exceed T-1.  Frame t of
    sequence n is observed iff t < n_obs[n].  Drawn on X's device from ``generator`` alone."""
    N, T = X.shape[0], X.shape[1]
    kmin, kmax, lead = int(kmin), int(kmax), int(lead)
    if lead < 1 or kmin <= lead or kmin > kmax or kmax > T:
        raise ValueError('ragged_frames: need lead < kmin <= kmax <= T, got lead=%d kmin=%d kmax=%d T=%d: the first %d frame(s) are '
                         'always kept and at least one later frame is drawn' % (lead, kmin, kmax, T, lead))
    dev = X.device
    k = torch.randint(kmin, kmax + 1, (N,), device=dev, generator=generator)
    # the k_n - lead smallest of T - lead uniform scores: a uniform subset, as in subsample_frames; a stable sort on "dropped" then
    # lists the kept frames first, in increasing order
    scores = torch.rand((N, T - lead), device=dev, generator=generator)
    rank = scores.argsort(dim=1).argsort(dim=1)
    keep = torch.cat((torch.ones((N, lead), dtype=torch.bool, device=dev), rank < (k[:, None] - lead)), dim=1)
    idx = (~keep).to(torch.int8).sort(dim=1, stable=True).indices[:, :kmax]
    col = torch.arange(kmax, device=dev)[None, :]
    obs = col < k[:, None]
    last = idx.gather(1, (k - 1)[:, None])             # idx[n, k_n - 1]
    idx = torch.where(obs, idx, last + (col - (k[:, None] - 1)))
    Xpad = X[torch.arange(N, device=dev)[:, None], idx.clamp(max=T - 1)]
    Xpad = torch.where(obs.view(N, kmax, *([1] * (X.dim() - 2))), Xpad, torch.zeros((), dtype=X.dtype, device=dev))
    return Xpad, idx, k.to(torch.int32)


class Dataset(data.Dataset):
    """Sequences (N, 16, 784) in [0, 1] -> items (16, 1, 28, 28), z-normalised (utils.py:5-15)."""

    def __init__(self, Xtr):
        self.Xtr = Xtr
        self.mean, self.std = MNIST_MEAN, MNIST_STD

    def __len__(self):
        return len(self.Xtr)

    def __getitem__(self, idx):
        item = torch.as_tensor(self.Xtr[idx], dtype=torch.float32).reshape(16, 1, 28, 28)
        return (item - self.mean) / self.std


class Dataset_labels(data.Dataset):
    """(frame, label) pairs; the label array is flattened (utils.py:17-28)."""

    def __init__(self, x, y):
        self.x, self.y = x, y.reshape(-1)

    def __len__(self):
        return self.y.shape[0]

    def __getitem__(self, index):
        return self.x[index], self.y[index]


class ResidentLoader:
    """Iterates minibatches of a tensor that stays on ``device``.  ``len()`` and the ragged last batch follow DataLoader
    (drop_last=False); ``shuffle`` draws one permutation per epoch from a device generator seeded with ``seed``."""

    def __init__(self, items, batch_size, shuffle=True, device='cuda', seed=0):
        self.items = items.to(device).contiguous()
        self.batch_size, self.shuffle = int(batch_size), shuffle
        self.gen = torch.Generator(device=self.items.device).manual_seed(seed)

    @property
    def dataset(self):
        return self.items

    def __len__(self):
        return (self.items.shape[0] + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = self.items.shape[0]
        order = torch.randperm(n, device=self.items.device, generator=self.gen) if self.shuffle else None
        for lo in range(0, n, self.batch_size):
            yield self.items[lo:lo + self.batch_size] if order is None else self.items.index_select(0, order[lo:lo + self.batch_size])
