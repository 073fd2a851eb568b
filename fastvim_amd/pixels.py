"""8-bit image batches: the loader's per-channel normalisation as a (C, 256) table, looked up inside the patch unfold.

Every loader of the reference starts from 8-bit pixels and normalises on the host before the batch reaches the device
(``ToTensor`` + ``Normalize`` in the ImageNet and MAE fine-tune / linear recipes; ``A.Normalize(mean / 255, std / 255)`` over
the 8 JUMP-CP channels, cell_imaging/config/FastChannelVimS.yaml:51-68).  With a table attached to the model's patch
embedding the static input buffer of a step object may hold the uint8 batch itself: a quarter of the host-to-device copy,
no float conversion on the host, and the unfold launch reads 150 KB per 224 px RGB image where it read 602 KB.

The arithmetic contract: a channel has 256 possible inputs, so the normalisation IS a table, and the HOST builds it with
torch in fp32 in the loader's own order of operations.  The kernels (csrc/unfold_u8.hip) only look values up -- the library
is built with -ffast-math, under which a kernel that computed ``(v / 255 - mean) / std`` would not be bit-identical to
the loader -- and from the looked-up fp32 value on do what the float kernels do.  The uint8 path therefore equals
"normalise on the host, then the float path" bit for bit, for fp32 and bf16 patches, with Mixup and without.

    pn = attach_pixel_norm(model, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    x = torch.empty(B, 3, 224, 224, device="cuda", dtype=torch.uint8)         # the step's static input buffer
    step = SegmentedTrainStep(model, flat, opt, mix.criterion(), x, labels, mixup=mix)
    x.copy_(batch_u8, non_blocking=True); ...; step.step()

Random erasing acts on the normalised image and therefore happens after the lookup, on the device:
``fastvim_amd.erasing.RandomErasing`` and ``SegmentedTrainStep(..., erase=re)``.

The MAE models (``fastvim_amd.models_mae``, ``fastvim_amd.fastvim_mae``) take uint8 batches as well: their reconstruction
loss looks the pixels up inside its own kernel (``fastvim_amd.losses.mae_reconstruction_loss``, csrc/mae_loss.hip).

Out of scope: RandAugment (a PIL stage: it stays 8-bit on the host) and channels-last batches (they take the eager lookup below
and then the float path, same values).
"""
import torch
import torch.nn.functional as F

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


class PixelNorm:
    """``mean`` / ``std`` per channel on the 0..1 scale (as the ImageNet configs write them; for the cell configs the caller
    passes the YAML values divided by 255, as cell.py:121-122 does).

    ``formula="torchvision"``:    ``table[c, v] = ((float32(v) / max_value) - mean[c]) / std[c]`` -- bit for bit what
    ``x.to(float32).div(255)``, ``sub_(mean)``, ``div_(std)`` give a uint8 tensor.
    ``formula="albumentations"``: ``table[c, v] = (float32(v) - mean[c] * max_value) * (1 / (std[c] * max_value))`` --
    ``A.Normalize``'s order (a reciprocal, then a product).  Everything in fp32, on the CPU (IEEE division)."""

    def __init__(self, mean, std, max_value=255.0, formula="torchvision"):
        mean_t = torch.as_tensor(mean, dtype=torch.float32).reshape(-1).clone()
        std_t = torch.as_tensor(std, dtype=torch.float32).reshape(-1).clone()
        if mean_t.numel() == 0 or mean_t.shape != std_t.shape:
            raise ValueError(f"PixelNorm: mean and std must have one value per channel, got {tuple(mean_t.shape)} and {tuple(std_t.shape)}")
        if not bool((std_t != 0).all()):
            raise ValueError("PixelNorm: std has a zero")
        if formula not in ("torchvision", "albumentations"):
            raise ValueError(f"PixelNorm: formula must be 'torchvision' or 'albumentations', got {formula!r}")
        self.mean, self.std, self.max_value, self.formula = mean_t, std_t, float(max_value), formula
        v = torch.arange(256, dtype=torch.uint8).to(torch.float32)[None, :].repeat(mean_t.numel(), 1)      # (C, 256)
        if formula == "torchvision":
            t = v.div(self.max_value).sub_(mean_t[:, None]).div_(std_t[:, None])
        else:
            t = v.sub_((mean_t * self.max_value)[:, None]).mul_(torch.reciprocal(std_t * self.max_value)[:, None])
        self._tables = {torch.device("cpu"): t.contiguous()}

    @property
    def channels(self):
        return self.mean.numel()

    def table(self, device="cpu"):
        """The (C, 256) fp32 table on ``device``, built once per device (a copy of the CPU table: no device arithmetic)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = self._tables[torch.device("cpu")].to(device)
        return t

    def __call__(self, x_u8):
        """Eager form: uint8 (B, C, H, W) -> fp32 normalised pixels by indexing the table.  The composition the kernels'
        predicates fall back to, and the reference of the tests."""
        return lookup(self.table(x_u8.device), x_u8)


def lookup(table, x_u8):
    """``out[b, c, y, x] = table[c, x_u8[b, c, y, x]]`` (fp32), any memory layout."""
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4:
        raise TypeError(f"pixel lookup: expected uint8 (B, C, H, W) images, got {tuple(x_u8.shape)} {x_u8.dtype}")
    C = x_u8.shape[1]
    if table.shape[0] != C:
        raise ValueError(f"pixel lookup: the table has {table.shape[0]} channel rows, the images have {C} channels")
    rows = torch.arange(C, device=x_u8.device, dtype=torch.int32).mul_(256).view(1, C, 1, 1)
    return F.embedding(x_u8.to(torch.int32) + rows, table.reshape(-1, 1)).squeeze(-1)


def _patch_embed_of(model):
    pe = getattr(model, "patch_embed", model)
    if not hasattr(pe, "proj") or not hasattr(pe, "patch_size"):
        raise TypeError(f"attach_pixel_norm: {type(model).__name__} has no patch embedding (`patch_embed`)")
    return pe


def embed_channels(pe):
    """Image channels a patch embedding takes: the conv's for ``PatchEmbed``, the channel-embedding table's rows for
    ``PatchEmbedPerChannel`` (whose shared filter has one input channel)."""
    ce = getattr(pe, "channel_embed", None)
    return ce.weight.shape[0] if ce is not None else pe.proj.weight.shape[1]


def attach_pixel_norm(model, mean, std, **kw):
    """Build ``PixelNorm(mean, std, **kw)`` and register its table on the model's patch embedding as the NON-persistent
    buffer ``pixel_table``: it follows ``model.to(device)``, and ``state_dict`` keys -- reference checkpoints -- are unchanged.
    From then on the model (``fastvim``, ``vim``, the channel models) takes uint8 (B, C, H, W) batches.  The table of a
    ``PatchEmbedPerChannel`` has ``in_chans`` rows and is indexed by the SOURCE channel.  Returns the ``PixelNorm``."""
    pe = _patch_embed_of(model)
    pn = PixelNorm(mean, std, **kw)
    if pn.channels != embed_channels(pe):
        raise ValueError(f"attach_pixel_norm: {pn.channels} channel statistics for a patch embedding of {embed_channels(pe)} channels")
    if "pixel_table" in pe._buffers:
        del pe._buffers["pixel_table"]
    pe.register_buffer("pixel_table", pn.table(pe.proj.weight.device).clone(), persistent=False)
    pe.pixel_norm = pn
    return pn


def pixel_table(pe, x):
    """The table attached to patch embedding ``pe`` for the uint8 batch ``x``, or the error that says what is missing."""
    table = getattr(pe, "pixel_table", None)
    if table is None:
        raise TypeError(f"{type(pe).__name__}: uint8 images need the normalisation table -- call "
                        "fastvim_amd.pixels.attach_pixel_norm(model, mean, std) first (float images are taken as normalised)")
    if table.shape[0] != x.shape[1]:
        raise ValueError(f"{type(pe).__name__}: the attached pixel table has {table.shape[0]} channel rows, the images have "
                         f"{x.shape[1]} channels")
    if table.device != x.device:
        raise RuntimeError(f"{type(pe).__name__}: the pixel table lives on {table.device}, the images on {x.device}")
    return table


def normalise_like(model, x_u8):
    """``PixelNorm.__call__`` with the table attached to ``model``'s patch embedding."""
    pe = _patch_embed_of(model)
    return lookup(pixel_table(pe, x_u8), x_u8)
