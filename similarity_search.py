#!/usr/bin/env python3
"""Similarity search entry point -- same CLI flags as the reference ``similarity_search.py``
(-tgt_fn -tst_fn -tgt_i -aug -mp -ct -snr -bs -m -c -dc -np -ns -dd) and the same ``.npz`` output
(``results/<model>_<target>_simsearch_results_f.npz`` with test_ra_decs, test_scores, target_images,
target_features, test_images, test_features).

Differences: figures are not drawn (matplotlib/LaTeX plotting is out of scope);
the 64x target augmentation (``-aug True``, the reference's default) runs on the device
(sky_embeddings_amd.augment: torchvision's parameter draws, one HIP launch per batch).  ``--bank`` (extension) encodes the
test set ONCE into a resident embedding bank and runs the fused cosine top-k kernel over it
instead of re-scoring streamed batches: one vector per sample with -mp True or -ct True, or, with both False, the
patch tokens of every sample scored one by one and combined per image (-c min | mean | max) by the fused token kernel;
``--bank-dtype f16 | bf16`` keeps that token bank in 16 bits (half the memory and half the bytes per search; the standardised
features are rounded once when stored).  ``-m MSE | MAE`` with ``--bank`` runs the fused distance kernel over the same resident bank in
all three modes (search.distance_topk_tokens; the pooled modes as a token bank with one token per sample, under that search's
limits: -ns <= 512 and a feature width that is a multiple of 64, at most 1024); ``test_scores`` are then distances, best
(smallest) first, as on the streamed path.  ``-nts / --n_top_sims T`` (extension) combines only the T best
patch scores of a sample (compute_similarity's n_top_sims): streamed without --bank, and with ``--bank -mp False -ct False``
inside the fused token kernel (1 <= T <= min(patches, 16)).  ``--bank-select-snr`` (extension, only with ``--bank``) encodes
EVERY row of the test file once and turns the ``-snr`` window into a selection of the resident bank (search.Selection; a 16-bit
cosine patch-token bank searches it on the two-stage many-query route when the window keeps at least 2048 token rows) instead
of filtering before the encoder: another S/N range is then another search over the same bank, not another encoding.  The
standardisation statistics are those of the first ``-bs`` SELECTED images (the reference's first batch of the filtered set; for
a 16-bit bank those images are encoded first to get them), results are looked up in the full test file.  It works in all three
--bank modes; the pooled ones (-mp True / -ct True) then run as the token search with one token per sample, under its limits:
-ns <= 512 and a feature width that is a multiple of 64, at most 1024.  ``--per-target`` (extension, only with ``--bank``) makes every
entry of ``-tgt_i`` its own query instead of pooling all targets into one mean vector and one weight vector: target t gets
``determine_target_features`` over its own latents alone (with ``-aug True`` its own 64 augmentations), i.e. its own inverse-variance
weights, and all targets are searched in one pass over the bank (search.* with ``weights`` [T, D]), in all three --bank modes and
with all three metrics.  The output is ``..._simsearch_results_per_target.npz``: the keys above with a leading target axis
(``test_scores`` [T, n_save], ...).  A target with fewer than two latent vectors (-aug False with -mp True / -ct True) has no
variance to weight by: the run exits with a message.
"""
import argparse
import ast
import configparser
import os

import numpy as np
import torch

from utils.dataloaders import build_h5_dataloader
from utils.eval_fns import build_embedding_bank, mae_latent
from utils.mim_vit import build_model as build_mim
from utils.misc import h5_snr, str2bool
from utils.similarity import determine_target_features, mae_simsearch
from utils.vit import build_model as build_vit


BANK_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
BANK_METRICS = ("cosine", "MSE", "MAE")


def parseArguments():
    parser = argparse.ArgumentParser('Similarity searching.', add_help=False)
    parser.add_argument("model_name", help="Name of model.", type=str)
    parser.add_argument("-tgt_fn", "--target_fn", type=str, default='HSC_dud_dwarf_galaxy_calexp_GIRYZ7610_64.h5')
    parser.add_argument("-tst_fn", "--test_fn", type=str, default='HSC_dud_unknown_calexp_GIRYZ7610_64.h5')
    parser.add_argument("-tgt_i", "--target_indices", default='[1,2]')
    parser.add_argument("-aug", "--augment_targets", type=str, default='True')
    parser.add_argument("-mp", "--max_pool", type=str, default='True')
    parser.add_argument("-ct", "--cls_token", type=str, default='False')
    parser.add_argument("-snr", "--snr_range", default='[2,7]')
    parser.add_argument("-bs", "--batch_size", type=int, default=64)
    parser.add_argument("-m", "--metric", type=str, default='cosine')
    parser.add_argument("-c", "--combine", type=str, default='min')
    parser.add_argument("-dc", "--display_channel", type=int, default=2)
    parser.add_argument("-np", "--n_plot", type=int, default=36)
    parser.add_argument("-ns", "--n_save", type=int, default=300)
    parser.add_argument("-dd", "--data_dir", help="Data directory if different from sky_embeddings/data/", type=str,
                        default=None)
    parser.add_argument("-nts", "--n_top_sims", type=int, default=None,
                        help="combine only the n best patch scores of a sample (-mp False -ct False)")
    parser.add_argument("--bank", action="store_true", help="encode once into a resident bank + fused top-k kernel")
    parser.add_argument("--bank-dtype", choices=sorted(BANK_DTYPES), default="f32",
                        help="element type of the resident patch-token bank (--bank -mp False -ct False)")
    parser.add_argument("--bank-select-snr", action="store_true",
                        help="with --bank: encode every test row once and apply -snr as a selection of the resident bank")
    parser.add_argument("--per-target", action="store_true",
                        help="with --bank: every -tgt_i entry is its own query with its own inverse-variance weights")
    return parser


def target_queries(tl, n_targets, per_target):
    """(queries [Q, D], weights) from the standardised target latents tl [n_targets * copies, tokens, D] (a target's copies are
    consecutive rows): one mean vector and one weight vector [D] over all of them, or, per target, [T, D] each from that target's
    own latents."""
    if not per_target:
        avg, w = determine_target_features(tl)
        return avg.reshape(1, -1), w
    groups = tl.reshape(n_targets, -1, tl.shape[-1])
    if groups.shape[1] < 2:
        raise SystemExit(f"--per-target: each target has {groups.shape[1]} latent vector, no variance to weight by (use -aug True, or "
                         f"-mp False -ct False)")
    pairs = [determine_target_features(g) for g in groups]
    return torch.stack([a for a, _ in pairs]), torch.stack([w for _, w in pairs])


def main():
    args = parseArguments().parse_args()
    target_indices = ast.literal_eval(args.target_indices) if args.target_indices != 'None' else None
    max_pool, cls_token = str2bool(args.max_pool), str2bool(args.cls_token)
    if (max_pool or cls_token) and args.n_top_sims not in (None, 1):
        raise SystemExit("-mp True / -ct True score one vector per sample: --n_top_sims must be 1 or left out")
    if args.bank and args.metric not in BANK_METRICS:
        raise SystemExit(f"--bank: unknown metric -m {args.metric}, expected one of {', '.join(BANK_METRICS)}")
    if args.bank_select_snr and not args.bank:
        raise SystemExit("--bank-select-snr selects images of the resident bank: it needs --bank")
    if args.per_target and not args.bank:
        raise SystemExit("--per-target searches the resident bank once for all targets: it needs --bank")
    snr_range = ast.literal_eval(args.snr_range)
    cur_dir = os.path.dirname(os.path.abspath(__file__))
    config_dir, model_dir = os.path.join(cur_dir, 'configs/'), os.path.join(cur_dir, 'models/')
    data_dir = args.data_dir if args.data_dir is not None else os.path.join(cur_dir, 'data/')
    results_dir = os.path.join(cur_dir, 'results/')
    os.makedirs(results_dir, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("similarity_search.py needs a GPU: the hot path is HIP-only (no CPU fallback)")
    device = torch.device('cuda')
    print(f'Using Torch version: {torch.__version__}')
    config = configparser.ConfigParser()
    config.read(config_dir + args.model_name + '.ini')
    model_filename = os.path.join(model_dir, args.model_name + '.pth.tar')
    if 'pretained_mae' in config['TRAINING']:
        mae_name = config['TRAINING']['pretained_mae']
        if mae_name == 'None':
            mae_filename, mae_config = 'None', config
        else:
            mae_config = configparser.ConfigParser()
            mae_config.read(config_dir + mae_name + '.ini')
            mae_filename = os.path.join(model_dir, mae_name + '.pth.tar')
        model, losses, cur_iter = build_vit(config, mae_config, model_filename, mae_filename, device)
    else:
        mae_config = config
        model, losses, cur_iter = build_mim(config, model_filename, device, build_optimizer=False)

    print('Estimating S/N for test dataset images...')
    test_snr = h5_snr(os.path.join(data_dir, args.test_fn), n_central_pix=8, batch_size=5000)
    test_snr = np.nanmin(test_snr[:, :5], axis=1)
    test_indices = np.where((test_snr > snr_range[0]) & (test_snr < snr_range[1]))[0]
    common = dict(batch_size=args.batch_size, num_workers=min(os.cpu_count(), 12),
                  img_size=int(config['ARCHITECTURE']['img_size']), num_patches=model.module.patch_embed.num_patches,
                  patch_size=int(mae_config['ARCHITECTURE']['patch_size']),
                  num_channels=int(mae_config['ARCHITECTURE']['num_channels']), max_mask_ratio=None, shuffle=False)
    target_dataloader = build_h5_dataloader(os.path.join(data_dir, args.target_fn), indices=target_indices, **common)
    # --bank-select-snr: every row is encoded, the S/N window becomes a selection of the bank
    test_dataloader = build_h5_dataloader(os.path.join(data_dir, args.test_fn),
                                          indices=None if args.bank_select_snr else test_indices, **common)
    target_latent, target_images = mae_latent(model, target_dataloader, device, return_images=True,
                                              apply_augmentations=str2bool(args.augment_targets), num_augmentations=64,
                                              remove_cls=False)
    if args.bank:
        from sky_embeddings_amd import search
        if args.bank_dtype != "f32" and (max_pool or cls_token):
            raise SystemExit("--bank-dtype f16 / bf16 applies to the patch-token bank (-mp False -ct False)")
        mod = model.module
        tl = target_latent.to(device)
        n_targets = tl.shape[0] // (65 if str2bool(args.augment_targets) else 1)     # a target and its 64 copies are consecutive
        k = args.n_save
        select, first_rows = None, slice(args.batch_size)
        if args.bank_select_snr:
            flags = torch.zeros(len(test_snr), dtype=torch.bool)
            flags[torch.from_numpy(test_indices)] = True
            select = search.Selection(flags, device)
            first_rows = torch.from_numpy(test_indices[:args.batch_size]).to(device)   # the first batch of the filtered set
            print(f'Selection: {select.count} of {select.N} test images inside the S/N window')
            if select.count == 0:
                raise SystemExit(f"--bank-select-snr: no test image has an S/N inside {snr_range}: nothing to search")
            k = min(k, select.count)         # the saved arrays line up: no (-inf, -1) tail
        if max_pool or cls_token:                # one vector per sample
            tl = tl[:, :1] if cls_token else tl[:, mod.num_extra_tokens:].max(dim=1, keepdim=True).values
            target_queries(tl, n_targets, args.per_target)     # too few latents per target: exit before the bank is encoded
            bank = build_embedding_bank(model, test_dataloader, device, pool='cls' if cls_token else 'max')
            first = bank[first_rows]         # the reference standardises with the first batch (utils/similarity.py:98-100)
            mean_feats, std_feats = first.mean(dim=0), first.std(dim=0, unbiased=True)
            tl = (tl - mean_feats) / (std_feats + 1e-8)
            search.standardise_(bank, mean_feats, std_feats)
            queries, w = target_queries(tl, n_targets, args.per_target)
            if args.metric == 'cosine':
                scores, idx = search.cosine_topk(queries, bank, min(k, bank.shape[0]), weights=w, select=select)
            else:                                # one token per sample: every combine is that token's distance
                scores, idx = search.distance_topk_tokens(queries, bank.unsqueeze(1), min(k, bank.shape[0]),
                                                          metric=args.metric, combine=args.combine, weights=w, select=select)
        else:                                    # every patch token scored, combined per image (-c min | mean | max)
            tl = tl[:, mod.num_extra_tokens:]
            if args.bank_dtype == "f32":
                bank = build_embedding_bank(model, test_dataloader, device, pool='tokens')
                first = bank[first_rows]         # mean / unbiased std over (batch, patch) of the first batch (utils/similarity.py:98-100)
                mean_feats, std_feats = first.mean(dim=(0, 1)), first.std(dim=(0, 1), unbiased=True)
                search.standardise_(bank.view(-1, bank.shape[2]), mean_feats, std_feats)
            else:                                # the same statistics; every batch standardised, rounded once and kept in 16 bits
                stats = None
                if select is not None:           # the first batch of the filtered set is encoded first, for its statistics
                    head = build_h5_dataloader(os.path.join(data_dir, args.test_fn), indices=test_indices[:args.batch_size], **common)
                    first = build_embedding_bank(model, head, device, pool='tokens', n_batches=1)
                    stats = (first.mean(dim=(0, 1)), first.std(dim=(0, 1), unbiased=True))
                bank, mean_feats, std_feats = build_embedding_bank(model, test_dataloader, device, pool='tokens',
                                                                   bank_dtype=BANK_DTYPES[args.bank_dtype],
                                                                   standardise_with_first_batch=True, standardise_stats=stats)
            print(f'Token bank: {bank.numel() * bank.element_size() / 1e9:.3f} GB, {bank.dtype}')
            tl = (tl - mean_feats) / (std_feats + 1e-8)
            queries, w = target_queries(tl, n_targets, args.per_target)
            if args.metric == 'cosine':
                if bank.dtype != torch.float32 and not args.per_target and bank.data_ptr() % 16 == 0:
                    # many targets over a 16-bit bank: the two-stage route where it applies, identical results by contract
                    tokens = search.TokenBank.resident(bank, w)
                else:
                    tokens = bank
                scores, idx = search.cosine_topk_tokens(queries, tokens, min(k, bank.shape[0]), combine=args.combine,
                                                        weights=w, top_t=args.n_top_sims, select=select)
            else:
                tokens = bank
                kk = min(k, bank.shape[0])
                if (bank.dtype != torch.float32 and bank.data_ptr() % 16 == 0
                        and search.token_mse_route_refusal(queries.shape[0], *bank.shape, kk, args.metric, args.combine, args.n_top_sims,
                                                           select is not None, args.per_target, top_t_prepared=True,
                                                           select_prepared=True,
                                                           selected=None if select is None else select.count,
                                                           per_query_prepared=True, mean_prepared=True) is None):
                    # many targets under weighted MSE over a 16-bit bank, and the two-stage route will take them (decided first: the
                    # wrapper costs a norm pass over the bank that the distance route never reads): identical results by contract.
                    # -nts, --bank-select-snr and --per-target take that route by opt-in, asked for here (--per-target: a second
                    # image of the bank, 4 bytes per element; its [T, D] weights travel with the search, not with the bank).
                    # -c mean takes it by opt-in as well: a pooled image of the bank, one pass, 2 D bytes per image
                    tokens = search.TokenBank.resident(bank, None if args.per_target else w)
                    if args.combine == 'mean':
                        tokens.prepare_mse_mean()
                    if args.per_target:
                        tokens.prepare_mse_per_query()
                    if args.n_top_sims:
                        tokens.prepare_mse_top_t()
                    if select is not None:
                        select.prepare_mse(tokens)
                scores, idx = search.distance_topk_tokens(queries, tokens, min(k, bank.shape[0]), metric=args.metric,
                                                          combine=args.combine, weights=w, top_t=args.n_top_sims, select=select)
        ds = test_dataloader.dataset

        def lookup(order):
            items = [ds[int(j)] for j in order if j >= 0]
            images = torch.stack([it[0] for it in items])
            return images, torch.stack([it[2] for it in items]), model.module.forward_features(images.to(device), reshape_out=False)[0]
        if args.per_target:                      # every array gains a leading target axis
            if bool((idx < 0).any()):
                raise SystemExit("--per-target: fewer than -ns images have a finite score for some target; lower -ns")
            rows = [lookup(order) for order in idx.cpu().numpy()]
            test_scores = scores
            test_images, test_ra_decs, test_latent = (torch.stack([r[j] for r in rows]) for j in range(3))
        else:
            test_scores = scores[0]
            test_images, test_ra_decs, test_latent = lookup(idx[0].cpu().numpy())
    else:
        test_images, test_latent, test_ra_decs, test_scores = mae_simsearch(
            model, target_latent, test_dataloader, device, metric=args.metric, combine=args.combine, use_weights=True,
            max_pool=max_pool, cls_token=cls_token, nested_batches=False, n_save=args.n_save, n_top_sims=args.n_top_sims)
    out = os.path.join(results_dir, f'{args.model_name}_{args.target_fn[:-3]}_simsearch_results_'
                                    f'{"per_target" if args.per_target else "f"}.npz')
    np.savez(out, test_ra_decs=test_ra_decs.cpu().numpy(), test_scores=test_scores.cpu().numpy(),
             target_images=target_images.cpu().numpy(), target_features=target_latent.cpu().numpy(),
             test_images=test_images.cpu().numpy(), test_features=test_latent.cpu().numpy())
    print('saved', out)


if __name__ == "__main__":
    main()
