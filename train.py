#!/usr/bin/env python3

"""Trains Karras et al. (2022) diffusion models: the single-GPU, single-process form of the reference's train.py.

The loss, its backward, the optimizer step (gradient clipping + AdamW + EMA + gradient zeroing, K.optim.AdamW), the sigma draw and the demo
sampler all run on this project's HIP kernels.  Differences from the reference, by design:
  * one process, one GPU; optimizer ``adamw`` only; no --gns, wandb or evaluation;
  * dataset types ``imagefolder``, ``imagefolder-class`` and ``custom`` go through a DataLoader (PIL, LANCZOS resize + centre crop; the class
    folders without torchvision: K.data.FolderOfImagesWithClasses); ``cifar10`` and ``mnist`` are read once from the files torchvision leaves on
    disk -- nothing is downloaded -- and kept on the device as uint8 (K.data.DeviceImageDataset): one HIP launch assembles each step's batch,
    there is no DataLoader, ``--num-workers`` is ignored and ``input_size`` must be the native 32 or 28; ``huggingface`` is refused;
  * conditioning dropout (``dataset.num_classes`` > 0, ``cond_dropout_rate``) runs on the device from this project's counter-based generator
    (K.data.class_dropout, or fused into the resident batch; one key per step from the default device generator -- not the reference's
    torch.rand);
  * augmentation (``augment_prob`` > 0) needs ``--device-augment``: the reference's KarrasAugmentationPipeline runs per image on the data-loader
    workers with scikit-image; here K.augmentation warps the uploaded batch on the device, with parameters from this project's counter-based
    generator (one key per step from the default device generator -- not the reference's torch draws).  Without the flag such a config is
    refused; with ``augment_prob`` 0, ``aug_cond`` is zeros [B, 9], what the reference's disabled pipeline yields;
  * both model families train: ``image_transformer_v2`` and the ``image_v1`` U-Net (bare, or in its augmentation wrapper, which is where
    ``aug_cond`` goes; a bare U-Net gets none).  ``check_model_config`` refuses, before a device is asked for, what the U-Net cannot take:
    class conditioning, augmentation without the wrapper, an ``input_size`` that some downsample cannot halve;
  * ``--mixed-precision bf16`` is the weight gradients' arithmetic alone (``model.set_wgrad_arithmetic('bf16')``: bf16 operands, fp32
    accumulation, on the trained model); everything else stays fp32;
  * a checkpoint also holds the RNG states and the position in the epoch, and the data order is a function of (seed, epoch), so that
    ``--resume`` continues the run it was saved from bit for bit (the reference restarts the epoch and its RNG streams).
"""

import argparse
from copy import deepcopy
import json
import math
import os
from pathlib import Path
import sys
import time
from types import SimpleNamespace

import torch
from torch.utils import data

import k_diffusion_amd as K


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--batch-size', type=int, default=64, help='the batch size')
    p.add_argument('--config', type=str, required=True, help='the configuration file')
    p.add_argument('--device-augment', action='store_true',
                   help="run the config's Karras augmentation (augment_prob > 0) on the device, on this project's HIP warp kernel")
    p.add_argument('--demo-every', type=int, default=500, help='save a demo grid every this many steps')
    p.add_argument('--end-step', type=int, default=None, help='the step to end training at')
    p.add_argument('--grad-accum-steps', type=int, default=1, help='the number of gradient accumulation steps')
    p.add_argument('--lr', type=float, help='the learning rate')
    p.add_argument('--name', type=str, default='model', help='the name of the run')
    p.add_argument('--num-workers', type=int, default=8, help='the number of data loader workers')
    p.add_argument('--reset-ema', action='store_true', help='reset the EMA')
    p.add_argument('--resume', type=str, help='the checkpoint to resume from')
    p.add_argument('--resume-inference', type=str, help='the inference checkpoint to resume from')
    p.add_argument('--sample-n', type=int, default=64, help='the number of images to sample for demo grids')
    p.add_argument('--save-every', type=int, default=10000, help='save every this many steps')
    p.add_argument('--seed', type=int, help='the random seed')
    # flags of the reference that this form does not implement: named, so that their use fails with a reason
    p.add_argument('--gns', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--wandb-project', type=str, help=argparse.SUPPRESS)
    p.add_argument('--evaluate-only', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--evaluate-every', type=int, default=0, help=argparse.SUPPRESS)
    p.add_argument('--evaluate-n', type=int, default=0, help=argparse.SUPPRESS)
    p.add_argument('--mixed-precision', type=str, help="'bf16': the weight-gradient GEMMs (and, for image_v1, convolutions) run on bf16 operands with fp32 accumulation")
    p.add_argument('--compile', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--checkpointing', action='store_true', help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.gns:
        p.error('--gns measures the gradient noise scale across DDP ranks; this is the single-GPU loop')
    if args.wandb_project:
        p.error('wandb logging is not implemented')
    if args.evaluate_only or args.evaluate_every > 0 or args.evaluate_n > 0:
        p.error('the evaluation flags are not implemented here: compute FID / KID with K.evaluation on samples of the checkpoint')
    if args.mixed_precision == 'bf16':
        args.mixed_precision, args.wgrad_bf16 = None, True
    else:
        args.wgrad_bf16 = False
    if args.mixed_precision or args.compile or args.checkpointing:
        p.error('--mixed-precision / --compile / --checkpointing are not implemented (the loss runs on the fp32 HIP path)')
    if args.grad_accum_steps < 1:
        p.error('--grad-accum-steps must be at least 1')
    return args


def make_grid(x, nrow):
    """[N, C, H, W] -> [C, rows * H, nrow * W], row-major, no padding (torchvision.utils.make_grid(x, nrow, padding=0))."""
    n, c, h, w = x.shape
    rows = math.ceil(n / nrow)
    grid = x.new_zeros(rows * nrow, c, h, w)
    grid[:n] = x
    return grid.view(rows, nrow, c, h, w).permute(2, 0, 3, 1, 4).reshape(c, rows * h, nrow * w)


def epoch_batches(n_items, batch_size, data_seed, epoch):
    """The epoch's batches (shuffle=True, drop_last=True) as a function of (data_seed, epoch)."""
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(data_seed + epoch)).tolist()
    return [perm[i:i + batch_size] for i in range(0, n_items - batch_size + 1, batch_size)]


DATASET_TYPES = ('imagefolder', 'imagefolder-class', 'cifar10', 'mnist', 'custom')
RESIDENT_TYPES = {'cifar10': (3, 32), 'mnist': (1, 28)}        # type -> (channels, native size): kept on the device as uint8


def check_dataset_config(config, class_emb_rows=None):
    """Refuses, with a reason, what the data path cannot do.  ``class_emb_rows``: the rows of the built model's class-embedding table
    (0 without one), checked against ``dataset.num_classes`` once the model exists."""
    dataset_config, model_config = config['dataset'], config['model']
    kind = dataset_config['type']
    num_classes = dataset_config.get('num_classes', 0)
    if kind == 'huggingface':
        raise NotImplementedError("dataset type 'huggingface' is not implemented: the datasets library is not a dependency; export the images "
                                  "to a folder (imagefolder / imagefolder-class) or wrap them in a custom dataset module")
    if kind not in DATASET_TYPES:
        raise ValueError(f'Invalid dataset type {kind!r}: one of {", ".join(DATASET_TYPES)}')
    if kind == 'imagefolder' and num_classes:
        raise NotImplementedError('dataset.num_classes > 0: an imagefolder dataset carries no class labels (use imagefolder-class)')
    if kind in RESIDENT_TYPES:
        channels, native = RESIDENT_TYPES[kind]
        if list(model_config['input_size']) != [native, native]:
            raise NotImplementedError(f'dataset type {kind!r} is kept on the device at its native {native} x {native}; input_size '
                                      f'{list(model_config["input_size"])} would need a resize of the resident array, which is not implemented '
                                      f'(export the images at that size to class folders and use imagefolder-class)')
        if model_config['input_channels'] != channels:
            raise ValueError(f'dataset type {kind!r} has {channels} channel(s); input_channels = {model_config["input_channels"]}')
    if class_emb_rows is not None and class_emb_rows != (num_classes + 1 if num_classes else 0):
        raise ValueError(f'dataset.num_classes = {num_classes} needs a class-embedding table of {num_classes + 1 if num_classes else 0} rows '
                         f'(num_classes + 1: the last row is the dropped label); the model has {class_emb_rows}')


def check_model_config(config):
    """Refuses, with a reason and before a device is asked for, a model section this command line cannot train.  Pure: it builds nothing.
    For ``image_v1``: class conditioning, augmentation without the wrapper that takes ``aug_cond``, and an ``input_size`` that some
    downsample cannot halve; ``patch_size``, ``skip_stages``, ``has_variance``, ``cross_cond_dim``, ``unet_cond_dim`` and the channel
    multiples are the constructor's refusals, by field name."""
    model_config, dataset_config = config['model'], config['dataset']
    if dataset_config.get('num_classes', 0) > 0:
        if model_config['type'] == 'image_v1':
            raise NotImplementedError('dataset.num_classes > 0 with model type image_v1: the U-Net takes no class_cond, so Denoiser.loss has '
                                      'nowhere to hand the labels; set dataset.num_classes to 0, or train an image_transformer_v2')
    if model_config['type'] != 'image_v1':
        return
    if model_config.get('augment_prob', 0) > 0 and not model_config.get('augment_wrapper', True):
        raise NotImplementedError('augment_prob > 0 with augment_wrapper: false: a bare image_v1 U-Net has nowhere for aug_cond to go; set '
                                  'augment_wrapper to true, or augment_prob to 0')
    K.models.image_v1.level_sizes(SimpleNamespace(depths=model_config['depths']), *model_config['input_size'])


def main(argv=None):
    args = parse_args(argv)

    config = K.config.load_config(args.config)
    model_config = config['model']
    dataset_config = config['dataset']
    opt_config = config['optimizer']
    sched_config = config['lr_sched']
    ema_sched_config = config['ema_sched']

    assert len(model_config['input_size']) == 2 and model_config['input_size'][0] == model_config['input_size'][1]
    size = model_config['input_size']
    augment_prob = model_config.get('augment_prob', 0)
    if augment_prob > 0 and not args.device_augment:
        raise NotImplementedError('augment_prob > 0: KarrasAugmentationPipeline (scikit-image warps) is not implemented; set augment_prob to 0, '
                                  'or pass --device-augment to augment each batch on the device (K.augmentation)')
    check_model_config(config)
    if opt_config['type'] != 'adamw':
        raise NotImplementedError(f'optimizer type {opt_config["type"]!r}: only adamw runs on the fused HIP step')
    check_dataset_config(config)
    if not torch.cuda.is_available():
        raise RuntimeError('train.py needs a ROCm device; there is no CPU fallback')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError('multi-GPU (DDP) training is not implemented: run one process on one device')
    device = torch.device('cuda')
    print(f'Using device: {device}', flush=True)
    print(f'Batch size: {args.batch_size}', flush=True)

    if args.seed is not None:
        seeds = torch.randint(-2 ** 63, 2 ** 63 - 1, [1], generator=torch.Generator().manual_seed(args.seed))
        torch.manual_seed(seeds[0])
    demo_gen = torch.Generator().manual_seed(torch.randint(-2 ** 63, 2 ** 63 - 1, ()).item())
    data_seed = torch.randint(0, 2 ** 62, ()).item()
    elapsed = 0.0

    inner_model = K.config.make_model(config)
    unet = model_config['type'] == 'image_v1'
    takes_aug_cond = not unet or model_config['augment_wrapper']        # the transformer, or the U-Net in its augmentation wrapper
    check_dataset_config(config, 0 if unet else inner_model.num_classes)          # the U-Net has no class-embedding table
    inner_model_ema = deepcopy(inner_model)
    print(f'Parameters: {K.utils.n_params(inner_model):,}')
    inner_model, inner_model_ema = inner_model.to(device), inner_model_ema.to(device)
    if any(rate > 0 for _, rate in inner_model._dropout_rates()):
        inner_model.enable_dropout()
    if args.wgrad_bf16:                              # the trained model only: the EMA copy never takes gradients
        inner_model.set_wgrad_arithmetic('bf16')
        if unet:
            print('Mixed precision bf16: the weight-gradient convolutions and GEMMs round their operands to bf16 (fp32 accumulation); the '
                  'forward pass, the loss, the data-gradient convolutions, AdaGN, the bias gradients, the attention rules, the optimizer and '
                  'the EMA stay fp32', flush=True)
        else:
            print('Mixed precision bf16: the weight-gradient GEMMs round their operands to bf16 (fp32 accumulation); the forward pass, the '
                  'loss, the data-gradient GEMMs, the attention rules, the optimizer and the EMA stay fp32', flush=True)

    lr = opt_config['lr'] if args.lr is None else args.lr
    opt = K.optim.AdamW(inner_model.param_groups(lr), lr=lr, betas=tuple(opt_config['betas']), eps=opt_config['eps'],
                        weight_decay=opt_config['weight_decay'])
    opt.attach_ema(inner_model, inner_model_ema)

    if sched_config['type'] == 'inverse':
        sched = K.utils.InverseLR(opt, inv_gamma=sched_config['inv_gamma'], power=sched_config['power'], warmup=sched_config['warmup'])
    elif sched_config['type'] == 'exponential':
        sched = K.utils.ExponentialLR(opt, num_steps=sched_config['num_steps'], decay=sched_config['decay'], warmup=sched_config['warmup'])
    elif sched_config['type'] == 'constant':
        sched = K.utils.ConstantLRWithWarmup(opt, warmup=sched_config['warmup'])
    else:
        raise ValueError('Invalid schedule type')

    assert ema_sched_config['type'] == 'inverse'
    ema_sched = K.utils.EMAWarmup(power=ema_sched_config['power'], max_value=ema_sched_config['max_value'])
    ema_stats = {}

    channels = model_config['input_channels']
    if channels not in (1, 3):
        raise NotImplementedError(f'the image datasets yield RGB or greyscale images; input_channels = {channels}')

    def tf(image):
        image = K.utils.resize_center_crop(image, size[0])
        return K.utils.from_pil_image(image if channels == 3 else image.convert('L'))

    image_key = dataset_config.get('image_key', 0)
    num_classes = dataset_config.get('num_classes', 0)
    cond_dropout_rate = dataset_config.get('cond_dropout_rate', 0.1)
    class_key = dataset_config.get('class_key', 1)

    resident = dataset_config['type'] in RESIDENT_TYPES
    if resident:                                     # the whole training set on the device as uint8; each step's batch is one launch
        read = K.data.read_cifar10 if dataset_config['type'] == 'cifar10' else K.data.read_mnist
        train_set = K.data.DeviceImageDataset(*read(dataset_config['location']), device=device, num_classes=num_classes or None)
        print(f'Dataset resident on the device ({train_set.images.numel() / 2 ** 20:.1f} MiB of uint8): no data loader, --num-workers is '
              f'ignored', flush=True)
    elif dataset_config['type'] == 'imagefolder':
        train_set = K.utils.FolderOfImages(dataset_config['location'], transform=tf)
    elif dataset_config['type'] == 'imagefolder-class':
        train_set = K.data.FolderOfImagesWithClasses(dataset_config['location'], transform=tf)
    else:
        train_set = K.data.load_custom(args.config, dataset_config, tf)
    print(f'Number of items in dataset: {len(train_set):,}')
    if len(train_set) < args.batch_size:
        raise ValueError(f'the dataset has {len(train_set)} images, fewer than one batch of {args.batch_size}')

    sigma_min = model_config['sigma_min']
    sigma_max = model_config['sigma_max']
    sample_density = K.training.make_sample_density(model_config)

    aug = K.augmentation.KarrasAugmentationPipeline(augment_prob) if augment_prob > 0 else None
    if aug is not None:
        print(f'Device augmentation: a_prob {augment_prob:g}', flush=True)

    model = K.config.make_denoiser_wrapper(config)(inner_model)
    model_ema = K.config.make_denoiser_wrapper(config)(inner_model_ema)

    state_path = Path(f'{args.name}_state.json')
    accum = args.grad_accum_steps
    epoch, step, batch_in_epoch = 0, 0, 0

    if state_path.exists() or args.resume:
        ckpt_path = args.resume if args.resume else json.load(open(state_path))['latest_checkpoint']
        print(f'Resuming from {ckpt_path}...')
        ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
        inner_model.load_state_dict(ckpt['model'])
        inner_model_ema.load_state_dict(ckpt['model_ema'])
        opt.load_state_dict(ckpt['opt'])
        sched.load_state_dict(ckpt['sched'])
        ema_sched.load_state_dict(ckpt['ema_sched'])
        ema_stats = ckpt.get('ema_stats', ema_stats)
        epoch, step = ckpt['epoch'], ckpt['step']
        if 'demo_gen' in ckpt:
            demo_gen.set_state(ckpt['demo_gen'])
        elapsed = ckpt.get('elapsed', 0.0)
        if 'rng_state' in ckpt:                      # a checkpoint of this script: continue its streams and its epoch
            torch.set_rng_state(ckpt['rng_state'])
            torch.cuda.set_rng_state(ckpt['cuda_rng_state'], device)
            data_seed, batch_in_epoch = ckpt['data_seed'], ckpt['batch_in_epoch']
            params = dict(inner_model.named_parameters())
            for n, g in ckpt.get('pending_grads', {}).items():
                params[n].grad = g.to(device)
        else:                                        # a reference checkpoint: it counts from the next epoch and step
            epoch, step = epoch + 1, step + 1
        del ckpt

    if args.reset_ema:
        inner_model.load_state_dict(inner_model_ema.state_dict())
        ema_sched = K.utils.EMAWarmup(power=ema_sched_config['power'], max_value=ema_sched_config['max_value'])
        ema_stats = {}

    if args.resume_inference:
        import safetensors.torch as safetorch
        print(f'Loading {args.resume_inference}...')
        ckpt = safetorch.load_file(args.resume_inference)
        inner_model.load_state_dict(ckpt)
        inner_model_ema.load_state_dict(ckpt)
        del ckpt

    @torch.no_grad()
    def demo():
        print('Sampling...', flush=True)
        filename = f'{args.name}_demo_{step:08}.png'
        with K.utils.eval_mode(model_ema):
            x = torch.randn([args.sample_n, channels, size[0], size[1]], generator=demo_gen).to(device) * sigma_max
            model_fn, extra_args = model_ema, {}
            if num_classes:
                extra_args['class_cond'] = torch.randint(0, num_classes, [args.sample_n], generator=demo_gen).to(device)
                model_fn = K.sampling.make_cfg_model_fn(model_ema, 1., num_classes)
            sigmas = K.sampling.get_sigmas_karras(50, sigma_min, sigma_max, rho=7., device=device)
            x_0 = K.sampling.sample_dpmpp_2m_sde(model_fn, x, sigmas, extra_args=extra_args, eta=0.0, solver_type='heun', disable=True)
        grid = make_grid(x_0, math.ceil(args.sample_n ** 0.5))
        K.utils.to_pil_image(grid.contiguous()).save(filename)

    def save():
        filename = f'{args.name}_{step:08}.pth'
        print(f'Saving to {filename}...', flush=True)
        obj = {
            'config': config,
            'model': inner_model.state_dict(),
            'model_ema': inner_model_ema.state_dict(),
            'opt': opt.state_dict(),
            'sched': sched.state_dict(),
            'ema_sched': ema_sched.state_dict(),
            'epoch': epoch,
            'step': step,
            'gns_stats': None,
            'ema_stats': ema_stats,
            'demo_gen': demo_gen.get_state(),
            'elapsed': elapsed,
            'rng_state': torch.get_rng_state(),
            'cuda_rng_state': torch.cuda.get_rng_state(device),
            'data_seed': data_seed,
            'batch_in_epoch': batch_in_epoch,
        }
        if step % accum != 0:                        # saved inside an accumulation window: the gradients gathered so far go along
            obj['pending_grads'] = {n: p.grad for n, p in inner_model.named_parameters() if p.grad is not None}
        torch.save(obj, filename)
        json.dump({'latest_checkpoint': filename}, open(state_path, 'w'))

    log = K.utils.CSVLogger(f'{args.name}_log.csv', ['step', 'epoch', 'time', 'loss', 'avg_loss', 'lr', 'ema_decay', 'grad_norm'])
    losses_since_last_print = []
    grad_norm = None

    try:
        while True:
            batches = epoch_batches(len(train_set), args.batch_size, data_seed, epoch)[batch_in_epoch:]
            if resident:
                train_dl = batches
            else:
                train_dl = data.DataLoader(train_set, batch_sampler=batches, num_workers=args.num_workers, pin_memory=True,
                                           generator=torch.Generator().manual_seed(data_seed + epoch)) if batches else ()
            for batch in train_dl:
                torch.cuda.synchronize()
                start_timer = time.time()

                sync_gradients = (step + 1) % accum == 0
                extra_args = {}
                # conditioning dropout: the key comes from the default device generator, so its state is in the checkpoint
                drop_key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=device) if num_classes else None
                if resident:
                    reals, class_cond = train_set.batch(batch, drop_key, cond_dropout_rate, num_classes)
                else:
                    reals = batch[image_key].to(device, non_blocking=True)
                    class_cond = K.data.class_dropout(batch[class_key].to(device, torch.int64), drop_key, cond_dropout_rate, num_classes) if num_classes else None
                if num_classes:
                    extra_args['class_cond'] = class_cond
                if aug is not None:                  # the key comes from the default device generator: its state is in the checkpoint
                    reals, _, aug_cond = aug.batch(reals)
                else:
                    aug_cond = reals.new_zeros([reals.shape[0], 9])
                if takes_aug_cond:
                    extra_args['aug_cond'] = aug_cond
                noise = torch.randn_like(reals)
                with K.utils.enable_stratified(step % accum, accum):
                    sigma = sample_density([reals.shape[0]], device=device)
                losses = model.loss(reals, noise, sigma, **extra_args)
                loss = losses.mean().item()
                losses_since_last_print.append(loss)
                (losses.mean() / accum).backward()
                ema_decay = ema_sched.get_value()
                if sync_gradients:
                    # clip at 1, AdamW, the EMA update and the gradient zeroing in one pass (train.py:463-467, :472)
                    grad_norm = opt.step(clip_grad_norm=1., ema_decay=ema_decay, zero_grad=True)
                sched.step()
                K.utils.ema_update_dict(ema_stats, {'loss': loss}, ema_decay ** (1 / accum))
                if sync_gradients:
                    ema_sched.step()

                torch.cuda.synchronize()
                elapsed += time.time() - start_timer

                log.write(step, epoch, elapsed, loss, ema_stats['loss'], sched.get_last_lr()[0], ema_decay,
                          '' if grad_norm is None else grad_norm.item())
                if step % 25 == 0:
                    loss_disp = sum(losses_since_last_print) / len(losses_since_last_print)
                    losses_since_last_print.clear()
                    print(f'Epoch: {epoch}, step: {step}, loss: {loss_disp:g}, avg loss: {ema_stats["loss"]:g}', flush=True)

                step += 1
                batch_in_epoch += 1

                if step % args.demo_every == 0:
                    demo()

                if step == args.end_step or (step > 0 and step % args.save_every == 0):
                    save()

                if step == args.end_step:
                    print('Done!')
                    return

            epoch += 1
            batch_in_epoch = 0
    except KeyboardInterrupt:
        pass


if __name__ == '__main__':
    sys.exit(main())
