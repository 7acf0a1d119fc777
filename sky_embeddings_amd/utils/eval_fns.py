"""utils/eval_fns.py mirror: ``mae_latent`` (encode a dataset into the embeddings that are searched, optionally with the
target augmentations), ``mae_predict`` (reconstructions), and the bank builder of SURVEY.md §8f rank 1.
``ft_predict``: the predictions of a trained downstream predictor."""
from __future__ import annotations

import numpy as np
import torch


def _net(model):
    return getattr(model, 'module', model)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def mae_predict(model, dataloader, device, mask_ratio, single_batch=True):
    """utils/eval_fns.py:9-70 -> (pred_imgs, masked_inputs, orig_imgs), NHWC numpy arrays in input units: predictions at
    the masked pixels, the input elsewhere; ``masked_inputs`` = the input with the masked pixels set to NaN."""
    net = _net(model)
    model.eval()
    if not single_batch:
        print(f'Reconstructing {len(dataloader)} batches')
    out = ([], [], [])
    with torch.no_grad():
        for samples, mask, ra_decs in dataloader:
            samples = samples.to(device, non_blocking=True)
            _, pred, mask = model(samples, ra_dec=ra_decs, mask_ratio=mask_ratio, mask=mask)
            if net.simmim:
                pred = pred.clone()                     # image-shaped already (SimMIM head + PixelShuffle index map)
            else:
                # per-patch rows -> image; the [B, L] patch mask -> pixel mask through the same un-patchify
                per_patch = net.patch_embed.patch_size[0] ** 2 * net.in_chans
                pred = net.unpatchify(pred)
                mask = net.unpatchify(mask.detach()[:, :, None].expand(-1, -1, per_patch))
            hidden = _nhwc(mask) == 1
            orig = _nhwc(samples)
            recon = torch.where(hidden, _nhwc(net.denorm_imgs(samples, pred)), orig)
            shown = torch.where(hidden, torch.full_like(orig, float('nan')), orig)
            for dst, t in zip(out, (recon, shown, orig)):
                dst.append(t.cpu().numpy())
            if single_batch:
                break
    return tuple(np.concatenate(parts) for parts in out)


def mae_latent(model, dataloader, device, n_batches=None, return_images=False, verbose=1, apply_augmentations=False,
               num_augmentations=16, remove_cls=True, augmentations=None):
    """utils/eval_fns.py:72-140: encoder-only forward of every batch -> latents [N, tokens, D] on the host.  With
    ``apply_augmentations`` every sample is followed by ``num_augmentations`` augmented copies (flip, resized crop,
    brightness, noise, NaN channels: utils/dataloaders.py:90-106) and its RA/Dec repeated for each -- produced by ONE
    device launch per batch (``Augmenter.batch``) instead of the reference's per-copy Python loop.  ``augmentations``
    overrides the pipeline (an ``Augmenter``, or any callable on one [C, H, W] tensor)."""
    net = _net(model)
    model.eval()
    limit = len(dataloader) if n_batches is None else min(n_batches, len(dataloader))
    if verbose > 0:
        print(f'Encoding {limit} batches' + (f' (+ {num_augmentations} augmented copies per sample)' if apply_augmentations else ''))
    if apply_augmentations and augmentations is None:
        from .dataloaders import get_augmentations
        augmentations = get_augmentations()         # crops are resized back to the sample's own size
    keep_from = 0 if (not remove_cls or net.attn_pool) else net.num_extra_tokens
    latents, images = [], []
    with torch.no_grad():
        for done, (samples, _masks, ra_decs) in enumerate(dataloader, 1):
            if apply_augmentations:
                copies = 1 + num_augmentations
                if hasattr(augmentations, 'batch'):
                    samples = augmentations.batch(samples, num_augmentations)
                else:   # a plain per-sample callable: original first, then its copies
                    samples = torch.stack([s if a == 0 else augmentations(s.clone()) for s in samples for a in range(copies)])
                ra_decs = ra_decs.repeat_interleave(copies, dim=0)
            samples = samples.to(device, non_blocking=True)
            latent = net.forward_features(samples, ra_dec=ra_decs, mask=None, reshape_out=False)[0]
            latents.append(latent[:, keep_from:].detach().cpu())
            if return_images:
                images.append(samples.detach().cpu())
            if done >= limit:
                break
    latents = torch.cat(latents)
    return (latents, torch.cat(images)) if return_images else latents


def build_embedding_bank(model, dataloader, device, pool='max', n_batches=None, bank_dtype=torch.float32,
                         standardise_with_first_batch=False, standardise_stats=None):
    """Encode a dataset ONCE into a resident [N, D] fp32 bank (cls token, or max / mean pool over
    the patch tokens -- all permutation invariant, so the reference's shuffled token order does not
    matter).  The reference re-encodes every test image per search (utils/similarity.py:81).
    ``pool='tokens'`` keeps the patch tokens themselves (extra tokens removed): a [N, P, D] bank for
    ``search.cosine_topk_tokens``.  The encoder returns them in shuffled order at mask_ratio = 0; the three combines
    over an image's tokens (min | mean | max of the token scores) do not depend on that order as sets -- min and max exactly,
    mean up to the rounding of its fixed-order fp32 sum.

    ``pool='tokens', bank_dtype=torch.float16 | torch.bfloat16, standardise_with_first_batch=True`` builds a half-precision
    resident bank without its fp32 image ever existing at full size: mean / unbiased std over (batch, patch) of the FIRST batch
    (as mae_simsearch takes them, utils/similarity.py:98-100), every batch standardised and rounded once to nearest-even
    (``search.standardise_to``), the 16-bit batches concatenated -> ``(bank, mean, std)``.  A 16-bit bank is stored
    standardised only: rounding raw features first would let ``standardise_`` amplify the rounding error.
    ``standardise_stats=(mean, std)`` replaces the first batch's statistics (those of another set of images, e.g. the first
    batch of a selection of this dataset).  The defaults return what they always returned."""
    from .. import search
    lp = bank_dtype != torch.float32
    if bank_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"build_embedding_bank: bank_dtype {bank_dtype} is not supported, expected torch.float32, torch.float16 or "
                         "torch.bfloat16")
    if standardise_stats is not None and not lp:
        raise ValueError("build_embedding_bank: standardise_stats applies to a 16-bit bank (standardise_with_first_batch=True)")
    if lp != bool(standardise_with_first_batch) or (lp and pool != 'tokens'):
        raise ValueError("build_embedding_bank: a 16-bit bank_dtype and standardise_with_first_batch=True go together, with "
                         "pool='tokens'")
    model.eval()
    net = _net(model)
    reduce = {'cls': lambda t: t[:, 0].clone(), 'max': lambda t: t[:, net.num_extra_tokens:].amax(dim=1),
              'mean': lambda t: t[:, net.num_extra_tokens:].mean(dim=1),
              'tokens': lambda t: t[:, net.num_extra_tokens:].to(torch.float32)}
    if pool not in reduce:
        raise ValueError(pool)
    rows = []
    with torch.no_grad():
        for done, (samples, _masks, ra_decs) in enumerate(dataloader, 1):
            feats = reduce[pool](net.forward_features(samples.to(device, non_blocking=True), ra_dec=ra_decs, reshape_out=False)[0])
            if lp:
                if done == 1:
                    mean, std = standardise_stats or (feats.mean(dim=(0, 1)), feats.std(dim=(0, 1), unbiased=True))
                feats = search.standardise_to(feats, mean, std, bank_dtype)
            rows.append(feats)
            if n_batches is not None and done >= n_batches:
                break
    if lp:
        return torch.cat(rows).contiguous(), mean, std
    return torch.cat(rows).contiguous()


def ft_predict(model, dataloader, device, num_batches=None, return_images=False, use_label_errs=False):
    """utils/eval_fns.py:142-192: predictions of a trained predictor (utils.vit) over a labelled loader, in label units
    (``denormalize_labels``) -> (tgt_labels, pred_labels[, images]) as numpy arrays.  With label errors the second half of the
    label columns is dropped.  (The reference stops after num_batches + 1 batches: kept.)"""
    model.eval()
    net = _net(model)
    tgt_labels, pred_labels, images = [], [], []
    if num_batches is None:
        num_batches = len(dataloader)
    print(f'Running predictions on {num_batches} batches...')
    with torch.no_grad():
        for i, (samples, masks, ra_decs, labels) in enumerate(dataloader):
            samples = samples.to(device, non_blocking=True)
            labels = labels.to(device, non_blocking=True)
            if use_label_errs:
                labels = labels[:, :labels.size(1) // 2]
            out = net.denormalize_labels(model(samples, mask=None, ra_dec=ra_decs.to(device, non_blocking=True)))
            tgt_labels.append(labels.cpu().numpy())
            pred_labels.append(out.float().cpu().numpy())
            if return_images:
                images.append(samples.cpu().numpy())
            if i == num_batches:
                break
    tgt_labels, pred_labels = np.concatenate(tgt_labels), np.concatenate(pred_labels)
    if return_images:
        return tgt_labels, pred_labels, np.concatenate(images)
    return tgt_labels, pred_labels
