"""Flags of the reference (argParser.py:3-73), same names and defaults, plus
the build's own: --data_root (Q8), --device, --mode,
--world_size, --n_max, --train_batch, --train_scenes, --valid_from_seed,
--log_dir, --save_dir, --seed, --use_grid_lstm, --loss, --num_samples,
--sample_seed, --head_log_sigma, --collision_radius, --fit_head,
--calibration, --fullcov_head, --mixture_head, --mixture_components,
--mixture_iters, --coupled_head, --kde_nll, --kde_floor, --sample_scores, --sample_ranks,
--rank_bins, --sample_kinematics, --kin_bins, --couple_scores, --couple_bins,
--couple_reach, --scene_ranks, --scene_bins, --scene_modes,
--scene_modes_iters, --sample_modes, --modes_draws, --modes_iters, --miss_radius."""
import argparse


class ArgsParser:
    parser = argparse.ArgumentParser()
    parser.add_argument('--input_size', type=int, default=2)
    parser.add_argument('--rnn_size', type=int, default=128)
    parser.add_argument('--num_layers', type=int, default=2)
    parser.add_argument('--model', type=str, default='lstm')
    parser.add_argument('--batch_size', type=int, default=16)
    parser.add_argument('--seq_length', type=int, default=12)
    parser.add_argument('--pred_len', type=int, default=12)
    parser.add_argument('--obs_len', type=int, default=8)
    parser.add_argument('--num_epochs', type=int, default=10)
    parser.add_argument('--save_every', type=int, default=50)
    parser.add_argument('--grad_clip', type=float, default=10.)
    parser.add_argument('--learning_rate', type=float, default=0.005)
    parser.add_argument('--decay_rate', type=float, default=0.95)
    parser.add_argument('--dropout', type=float, default=0.8)
    parser.add_argument('--embedding_size', type=int, default=64)
    parser.add_argument('--neighborhood_size', type=int, default=64)
    parser.add_argument('--grid_size', type=int, default=4)
    parser.add_argument('--num_freq_blocks', type=int, default=10)
    parser.add_argument('--maxNumPeds', type=int, default=20)
    parser.add_argument('--leaveDataset', type=int, default=2)
    parser.add_argument('--lambda_param', type=float, default=0.0005)
    # build additions
    parser.add_argument('--data_root', type=str, default='data',
                        help='directory holding eth/ and ucy/ (replaces hard-coded paths, Q8)')
    parser.add_argument('--device', type=str, default='cuda')
    parser.add_argument('--mode', choices=('reference', 'train'), default='reference',
                        help="reference: train.py's legs (no loss, as the reference); train: "
                             "RMSProp on the L2 loss over the fold's real scenes, data parallel")
    parser.add_argument('--world_size', type=int, default=0,
                        help='--mode train: expected ranks (torchrun WORLD_SIZE; 0: any)')
    parser.add_argument('--n_max', type=int, default=0,
                        help='--mode train: pedestrian padding Nmax (0: the largest scene, '
                             'rounded up to 16; larger scenes are left out)')
    parser.add_argument('--train_batch', type=int, default=256,
                        help='--mode train: scenes per global step (a multiple of the ranks)')
    parser.add_argument('--loss', choices=('l2', 'nll'), default='l2',
                        help='--mode train: 1/2 squared error of the predictions, or the '
                             'bivariate-Gaussian NLL with a learned per-step head')
    parser.add_argument('--num_samples', type=int, default=0,
                        help='best-of-K sampling evaluation on the left-out dataset with K draws '
                             'of the Gaussian head (minADE_K / minFDE_K; --mode train runs it after '
                             'the last epoch; 0: off)')
    parser.add_argument('--sample_seed', type=int, default=0,
                        help='--num_samples: seed of draw 0 (draw k uses seed + k)')
    parser.add_argument('--head_log_sigma', type=float, default=0.0,
                        help="--num_samples: log sigma of the head when the parameters hold none "
                             "(an L2-trained checkpoint)")
    parser.add_argument('--collision_radius', type=float, default=0.0,
                        help='--num_samples: also report the joint best-of-K figures (JADE_K / '
                             'JFDE_K) and the collision rates: two pedestrians collide when they '
                             'come closer than this at any predicted step, in the units of the '
                             "dataset's position columns (0: off)")
    parser.add_argument('--fit_head', choices=('off', 'train', 'eval'), default='off',
                        help='--num_samples: before the draws, replace the head by the closed-form '
                             "maximum-likelihood fit of the residuals on the scenes of the fold's "
                             'training datasets (train; honours --train_scenes) or of the left-out '
                             'dataset itself (eval: in-sample, a bound).  eth_hotel is normalised to '
                             '0..1 and the UCY sets are world coordinates, so a pooled fit mixes '
                             'the two units')
    parser.add_argument('--calibration', type=int, default=0,
                        help='--num_samples: 1 reports the calibration of the head in use on the '
                             'left-out dataset (NLL per pair, coverage of the 50 / 90 / 95 %% '
                             'ellipses, ECE, mean(q) / 2); implied by --fit_head train / eval')
    parser.add_argument('--fullcov_head', choices=('off', 'train', 'eval'), default='off',
                        help='--num_samples: after the per-step figures, also fit the full-covariance '
                             'trajectory head (one Gaussian over the 24 residuals of a pedestrian, so '
                             "a draw is a correlated trajectory) on the scenes of the fold's training "
                             'datasets (train; honours --train_scenes) or of the left-out dataset '
                             'itself (eval: in-sample, a bound), and report its minADE_K / minFDE_K, '
                             'joint NLL, coverage and the lag-1 correlation of the residuals')
    parser.add_argument('--mixture_head', choices=('off', 'train', 'eval'), default='off',
                        help='--num_samples: after --fullcov_head\'s figures, also fit the '
                             'Gaussian-mixture trajectory head (--mixture_components full-covariance '
                             'Gaussians over the 24 residuals, by --mixture_iters EM iterations on the '
                             "device) on the scenes of the fold's training datasets (train; honours "
                             '--train_scenes) or of the left-out dataset itself (eval: in-sample, a '
                             'bound), and report its minADE_K / minFDE_K, NLL per pair, live '
                             'components, largest weight and the log-likelihood gained by EM')
    parser.add_argument('--mixture_components', type=int, choices=range(1, 9), default=3,
                        metavar='1..8', help='--mixture_head: components of the mixture')
    parser.add_argument('--mixture_iters', type=int, default=30,
                        help='--mixture_head: EM iterations')
    parser.add_argument('--coupled_head', choices=('off', 'train', 'eval'), default='off',
                        help='--num_samples: after --mixture_head\'s figures, also fit the scene-coupled '
                             'head (the Gaussian whose joint draws share a part among the pedestrians of '
                             "a scene-frame; closed form) on the scenes of the fold's training datasets "
                             '(train; honours --train_scenes) or of the left-out dataset itself (eval: '
                             'in-sample, a bound), and report the shared part of the residual variance, '
                             'its joint NLL per pair and what the coupling gains over the independent '
                             'head with the same marginals; with --collision_radius / --couple_scores '
                             'also its joint figures and couple-distance scores')
    parser.add_argument('--kde_nll', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (K >= 4): 1 also reports the KDE-NLL of the K draws '
                             '(per step a Gaussian kernel density estimate of the drawn positions, '
                             "Scott's bandwidth, and the target's negative log density under it), "
                             'of the per-step head and, with --fullcov_head, of the '
                             'full-covariance head')
    parser.add_argument('--kde_floor', type=float, default=-20.0,
                        help='--kde_nll: the floor of a step\'s log density')
    parser.add_argument('--sample_scores', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (2 <= K <= 256): 1 also reports the energy scores '
                             '(24-D norm, ADE, FDE), the expected ADE / FDE of a draw, the average '
                             'pairwise displacement and the variogram score of the K draws, of the '
                             'per-step head and, with --fullcov_head / --mixture_head, of those heads')
    parser.add_argument('--sample_ranks', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (4 <= K <= 255): 1 also reports the rank-histogram '
                             "calibration of the K draws (the target's rank among the draws per step "
                             'and per trajectory, uniform when calibrated: distance from uniform, '
                             'mean rank, coverage at 50 / 90 %%), of the per-step head and, with '
                             '--fullcov_head / --mixture_head, of those heads')
    parser.add_argument('--rank_bins', type=int, default=0,
                        help='--sample_ranks: bins of the histograms, a divisor of K + 1 up to 64 '
                             '(0: the largest divisor <= 32)')
    parser.add_argument('--sample_kinematics', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (2 <= K <= 255): 1 also reports the kinematic scores of '
                             'the K draws (per group of features, speed / acc / lacc / straight in the '
                             "dataset's units per step: the fair CRPS, the target's mean PIT rank among "
                             "the draws, the PIT histogram's distance from uniform, the draws' and the "
                             "targets' mean feature), of the per-step head and, with --fullcov_head / "
                             '--mixture_head, of those heads')
    parser.add_argument('--kin_bins', type=int, default=0,
                        help='--sample_kinematics: bins of the PIT histograms, a divisor of K + 1 up to '
                             '64 (0: the largest divisor <= 32)')
    parser.add_argument('--couple_scores', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (2 <= K <= 64): 1 also reports the couple-distance scores '
                             'of the K draws taken as joint samples (per couple of pedestrians of a '
                             'scene, the closest approach and the final separation: the fair CRPS, the '
                             "targets' mean PIT rank among the draws, the PIT histogram's distance from "
                             "uniform, the draws' and the targets' mean), of the per-step head and, "
                             'with --fullcov_head / --mixture_head, of those heads')
    parser.add_argument('--couple_bins', type=int, default=0,
                        help='--couple_scores: bins of the PIT histograms, a divisor of K + 1 up to 64 '
                             '(0: the largest divisor <= 32)')
    parser.add_argument('--couple_reach', type=float, default=0.0,
                        help="--couple_scores: score the couples whose mean predictions come closer "
                             "than this, in the dataset's own units as --collision_radius (0: every "
                             'couple)')
    parser.add_argument('--scene_ranks', type=int, choices=(0, 1), default=0,
                        help='--num_samples K (2 <= K <= 64): 1 also reports the scene-level rank '
                             "calibration of the K draws taken as joint samples (a scene's targets "
                             'ranked among the draws by typicality, common mode and within-scene '
                             "spread: the rank histograms' distance from uniform and the mean PIT, "
                             "the draws' and the targets' mean feature, and the fair energy score of "
                             "the scene's joint law), of the per-step head and, with --fullcov_head / "
                             '--mixture_head / --coupled_head, of those heads')
    parser.add_argument('--scene_bins', type=int, default=0,
                        help='--scene_ranks: bins of the rank histograms, a divisor of K + 1 up to 64 '
                             '(0: the largest divisor <= 32)')
    parser.add_argument('--scene_modes', type=int, default=0,
                        help='--num_samples K (max(M, 2) <= K <= 64): M in 1..32 also reduces the K draws '
                             'taken as joint samples of a scene to M scene modes, each one of the draws '
                             'with a probability (k-medoids in double precision), and reports '
                             'minJADE_M / minJFDE_M of the modes, their Brier variants, the scene-level '
                             'miss rate at --miss_radius, the clustering cost and the minJADE of the '
                             'first M raw draws and of all K, of the per-step head and, with '
                             '--fullcov_head / --mixture_head / --coupled_head, of those heads (0: off)')
    parser.add_argument('--scene_modes_iters', type=int, default=10,
                        help='--scene_modes: alternating rounds after the start, at most, 0..32')
    parser.add_argument('--sample_modes', type=int, default=0,
                        help='--num_samples: M in 1..32 also reduces --modes_draws draws of each head '
                             'in use to M representative trajectories with probabilities (k-means '
                             'over the 24-D trajectories of a pedestrian) and reports minADE_M / '
                             'minFDE_M of the centres, their Brier variants, the inertia and the '
                             'live clusters (0: off)')
    parser.add_argument('--modes_draws', type=int, default=256,
                        help='--sample_modes M: draws clustered per pedestrian, M..256 (seed '
                             '--sample_seed: the first --num_samples are the best-of-K draws)')
    parser.add_argument('--modes_iters', type=int, default=10,
                        help="--sample_modes: iterations of Lloyd's algorithm, 0..64")
    parser.add_argument('--miss_radius', type=float, default=0.0,
                        help='--sample_modes: also report the miss rate, the share of pedestrians '
                             'whose best centre ends farther than this from the target, in the units '
                             "of the dataset's position columns (0: off)")
    parser.add_argument('--train_scenes', type=int, default=0,
                        help='--mode train: distinct scenes used (0: all of the fold)')
    parser.add_argument('--valid_from_seed', type=int, default=0,
                        help="validation leg from the file's first frame (the reference starts "
                             "at frame 0, which the ETH/UCY frame keys never hit)")
    parser.add_argument('--use_grid_lstm', type=int, default=0,
                        help="run the vis/loc encoder's GridLSTMCell in every frame and feed its "
                             "output as st_embeddings (train.py:201-207; 0: the reference, whose "
                             "encoder outputs are overridden by feeds, quirk Q5)")
    parser.add_argument('--log_dir', type=str, default='log')
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--save_dir', type=str, default='',
                        help='write TF-bundle checkpoints every --save_every batches (train.py:330-343)')
