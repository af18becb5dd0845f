"""The reference's image loader (code/datasets/jpg_dataloader.py) restated with plain torch CPU ops:
the reference of the image-ingest tests.  torchvision is not installed, so ``val_transforms``
(:164-171) is written out in its arithmetic; this parity is pinned by restatement."""
import torch

MEAN = [0.485, 0.456, 0.406]      # :168
STD = [0.229, 0.224, 0.225]       # :169


def to_tensor_normalize(img):
    """``Compose([ToTensor(), Normalize(MEAN, STD)])`` of one HWC uint8 image -> CHW fp32:
    ``permute -> .to(float32).div(255)``, then ``sub_(mean).div_(std)`` with fp32 mean / std."""
    x = torch.as_tensor(img).permute(2, 0, 1).contiguous().to(dtype=torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return x.sub_(mean).div_(std)


def get_data(bag):
    """``get_data`` (:229-257) over already decoded tiles [n, H, W, 3]: the stacked transforms."""
    bag = torch.as_tensor(bag)
    if bag.shape[0] == 0:
        return torch.zeros(0, 3, bag.shape[1], bag.shape[2])
    return torch.stack([to_tensor_normalize(t) for t in bag])


def to_fixed_size_bag(bag, coords, bag_size):
    """``to_fixed_size_bag`` (:284-293): one randperm on the default generator, zero tiles after."""
    idx = torch.randperm(bag.shape[0])[:bag_size]
    samples = bag[idx]
    padded = torch.cat((samples, torch.zeros(bag_size - samples.shape[0], *samples.shape[1:])))
    return padded, coords[idx]


def getitem(bag, coords, mode, bag_size):
    """``__getitem__`` (:306-361) without the label / names: (tiles fp32, coords)."""
    x = get_data(bag)
    if mode in ("train", "val"):
        return to_fixed_size_bag(x, coords, bag_size)
    return x, coords


def random_bags(sizes, H, W, seed):
    """Seeded uint8 bags [n_i, H, W, 3] and int64 coords [n_i, 2]."""
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g) for n in sizes]
    coords = [torch.randint(0, 50000, (n, 2), dtype=torch.int64, generator=g) for n in sizes]
    return bags, coords
