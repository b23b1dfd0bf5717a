"""Multimodal evaluation: best-of-K sampling on the left-out dataset
(minADE_K / minFDE_K, the usual figure of a probabilistic predictor on
ETH/UCY at K = 20).

  python -m multimodaltraj_2_amd.evaluate --data_root D --save_dir DIR \
      --leaveDataset l --num_samples 20 [--sample_seed N]

Every distinct scene of dataset l (realdata.plan_scenes: sample.py's scene per
frame pointer, as --mode train takes them from the training datasets) goes
through ONE fused step (g2k_step_fused_f32, stride 0, one frame: a real
scene's prediction is the same in every frame of its loop, so each (scene,
pedestrian) counts once, not once per frame) and ONE g2k_best_of_k_f32 launch
over its predictions: K draws of the Gaussian head around each prediction,
the smallest ADE and FDE per pedestrian, no draw ever in memory
(csrc/g2k_bestk.hip).  With --collision_radius R > 0 one g2k_joint_eval_f32
launch (csrc/g2k_joint.hip) follows on the same predictions, head and seed:
the K draws taken as joint samples of a scene (JADE_K / JFDE_K: one k for all
pedestrians of the scene, so never below minADE_K / minFDE_K) and the share of
pedestrian couples that come closer than R at any of the 12 predicted steps —
in the K samples, in the mean prediction, in each scene's best joint sample
and in the ground truth.  R is in the units realdata.plan_scenes hands the
kernels: the position columns of the dataset's CSV as they are, neither
normalised nor shifted — for the UCY sets (zara01, zara02, ucy_univ) world
coordinates spanning about -9..5 by -3..3, for eth_hotel image coordinates
normalised to 0..1.  The head is the checkpoint's (``nll_head/head``, which
--mode train --loss nll learns) or, for parameters without one, a constant
exp(--head_log_sigma) per step.  All of these figures depend on how wide that
head is, so --fit_head train / eval replaces it, before the first draw, by the
closed-form maximum-likelihood head of the residuals (GaussianHead.fit, one
g2k_head_stats_f32 launch, csrc/g2k_calib.hip) over the scenes of the fold's
training datasets (one more fused step over them) or over the left-out scenes
themselves (in-sample: a bound, not an estimate), and --calibration 1 (implied
by --fit_head) reports how the head in use fits the left-out scenes: NLL per
pair, the share of targets inside its 50 / 90 / 95 % ellipses, the expected
calibration error over the levels 0.1 .. 0.9, 0.95, 0.99 and mean(q) / 2 (1
when calibrated).  --fullcov_head train / eval then fits, after all of the
above and on the same predictions, K and seed, the full-covariance trajectory
head (fullcov.FullCovHead, csrc/g2k_fullcov.hip: one Gaussian over a
pedestrian's 24 residuals, so that a draw is a temporally correlated
trajectory and not 12 independent steps) and reports its minADE_K / minFDE_K,
joint NLL per pair, the share of trajectories inside its 90 % region, sum q /
24 n and the mean correlation of the x-residuals at adjacent steps: how far
from independent the steps are.  With --collision_radius R > 0 as well, one
g2k_fullcov_joint_eval_f32 launch (csrc/g2k_joint.hip) follows: the
same K correlated draws taken as joint samples (FULLCOV_JOINT_FIGURES: JADE_K,
JFDE_K, the collision rate of the samples and of each scene's best joint
sample), logged next to the per-step head's.  --kde_nll 1 (K >= 4) adds the
KDE-NLL of the same K draws, one g2k_kde_nll_f32 launch (csrc/g2k_kde.hip): per
pedestrian and step a Gaussian kernel density estimate of the K drawn positions
(Scott's bandwidth, scipy.stats.gaussian_kde's default) and the target's
negative log density under it, floored at --kde_floor (KDE_FIGURES: the mean
over the 12 steps, the last step's, and the share of steps on the floor) — the
one likelihood figure with the same definition for both heads, so with
--fullcov_head a g2k_fullcov_kde_nll_f32 launch adds FULLCOV_KDE_FIGURES; unlike
minADE_K it grows when the head is too wide.  --sample_scores 1 (2 <= K <= 256)
adds the trajectory-level scores of the same K draws, one g2k_sample_scores_f32
launch per head (csrc/g2k_scores.hip; SCORE_FIGURES): the fair energy score with
the 24-D norm (strictly proper for the joint law of the 12 steps), with the ADE
and the FDE (marginals only), the expected ADE / FDE of a draw, the average
pairwise displacement and the variogram score of order 1/2, which is the one
that sees whether a draw zig-zags.  --sample_modes M (1 <= M <= 32) reduces
--modes_draws draws (default 256, seed --sample_seed: the first --num_samples
of them are the best-of-K call's own) of each head in use to M representative
trajectories with probabilities, one g2k_sample_modes_f32 launch per head
(csrc/g2k_modes.hip: --modes_iters rounds of Lloyd's algorithm in double
precision), and reports MODES_FIGURES: minADE_M / minFDE_M of the centres,
their Brier variants with the clusters' weights, the inertia and the number of
live clusters, and with --miss_radius R > 0 (the dataset's own units, as
--collision_radius) the share of pairs whose best centre ends farther than R
from the target.  --sample_ranks 1 (4 <= K <= 255) adds the rank-histogram
calibration of the same K draws, one g2k_sample_ranks_f32 launch per head in use
(csrc/g2k_ranks.hip; RANK_FIGURES): the target pooled with the draws and ranked
among them, per step by a kernel density and per trajectory by the energy
distance, in --rank_bins bins (0: the largest divisor of K + 1 up to 32) — the
distance of the histograms from uniform, the mean rank (1/2 when calibrated;
the steps' above 1/2: the head is too narrow) and the share of targets among
the 50 / 90 % most typical points: one definition for the three heads, and the
mixture head's only coverage figure.  --sample_kinematics 1 (2 <= K <= 255) adds
the kinematic scores of the same K draws, one g2k_sample_kin_f32 launch per head
in use (csrc/g2k_kin.hip; KIN_FIGURES): per group of features — speed, acc,
lacc (longitudinal acceleration) and straight, in the dataset's units per 0.4 s
step — the fair CRPS, the mean PIT rank of the target among the draws (1/2 when
calibrated; below it: the draws' feature is larger than the target's), the
distance of the PIT histogram from uniform in --kin_bins bins, and the draws'
and the targets' mean feature.  --couple_scores 1 (2 <= K <= 64) adds the
couple-distance scores of the same K draws taken as JOINT samples, one
g2k_couple_scores_f32 call per head in use (csrc/g2k_couples.hip; CPL_FIGURES):
per couple of a scene-frame's members whose mean predictions come within
--couple_reach (0: every couple) the closest approach ("min") and the final
separation ("fin") — the fair CRPS, the mean PIT rank of the targets' among the
draws' (1/2 when calibrated), the distance of the PIT histogram from uniform in
--couple_bins bins, and the draws' and the targets' mean: the one proper score
here of how the pedestrians depend on each other.  --scene_ranks 1 (2 <= K <=
64) adds the scene-level rank calibration of the same joint draws, one
g2k_scene_ranks_f32 call per head in use (csrc/g2k_scene_ranks.hip;
SCN_FIGURES): the targets' whole configuration of a scene ranked among the
draws' by typicality, common mode and within-scene spread in --scene_bins bins,
and the fair energy score of the scene's joint law, which is reported and never
gated on (it hardly sees dependence).  --scene_modes M (1 <= M <= 32, max(M, 2)
<= K <= 64) reduces the same joint draws of every scene to M scene modes, each
one of the draws with a probability, one g2k_scene_modes_f32 call per head in
use (csrc/g2k_scene_modes.hip: k-medoids in double precision,
--scene_modes_iters rounds; SMD_FIGURES): minJADE_M / minJFDE_M of the modes,
their Brier variants, the scene-level miss rate at --miss_radius, the
clustering cost, and the minJADE of the first M raw draws and of all K.
--coupled_head train / eval
fits the one head that MODELS that dependence (coupled.CoupledHead,
csrc/g2k_coupled.hip: r = c + e, c shared by the members of a scene-frame;
closed form) and reports the shared part of the residual variance, its exact
joint NLL per pair, what that gains over the independent head with the same
marginals and the two calibration ratios (COUPLED_FIGURES), and with the two
flags above its joint figures and couple-distance scores.  The units caveat above holds for a pooled
fit too: eth_hotel is normalised, the UCY sets are world coordinates, so a fold
that mixes them fits one width to both.  The build's: the reference has no probabilistic head
(SURVEY.md §8(f) row 4), so these figures have no reference counterpart.
"""
from __future__ import annotations

import numpy as np
import torch

from . import checkpoint
from . import frame_step as fs
from . import realdata as rd
from .nll import GaussianHead

FIGURES = ("ade", "fde", "min_ade", "min_fde")
JOINT_FIGURES = ("jade", "jfde", "ped_pairs", "collision_rate", "collision_rate_pred",
                 "collision_rate_best", "collision_rate_gt")
CALIB_FIGURES = ("nll", "coverage_50", "coverage_90", "coverage_95", "ece", "q_ratio")
CALIB_LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)
FULLCOV_FIGURES = ("fullcov_min_ade", "fullcov_min_fde", "fullcov_nll", "fullcov_coverage_90",
                   "fullcov_q_ratio", "fullcov_lag1_corr")
FULLCOV_JOINT_FIGURES = ("fullcov_jade", "fullcov_jfde", "fullcov_collision_rate",
                         "fullcov_collision_rate_best")
KDE_FIGURES = ("kde_nll", "kde_nll_final", "kde_clipped")
FULLCOV_KDE_FIGURES = tuple("fullcov_" + k for k in KDE_FIGURES)
MIX_FIGURES = ("mix_min_ade", "mix_min_fde", "mix_nll", "mix_components", "mix_weight_max",
               "mix_loglik_gain")
MIX_JOINT_FIGURES = ("mix_jade", "mix_jfde", "mix_collision_rate", "mix_collision_rate_best")
MIX_KDE_FIGURES = tuple("mix_" + k for k in KDE_FIGURES)
SCORE_FIGURES = ("es_traj", "es_ade", "es_fde", "mean_ade", "mean_fde", "apd", "vs")
FULLCOV_SCORE_FIGURES = tuple("fullcov_" + k for k in SCORE_FIGURES)
MIX_SCORE_FIGURES = tuple("mix_" + k for k in SCORE_FIGURES)
MODES_FIGURES = ("modes_min_ade", "modes_min_fde", "modes_brier_ade", "modes_brier_fde", "modes_inertia",
                 "modes_live")
FULLCOV_MODES_FIGURES = tuple("fullcov_" + k for k in MODES_FIGURES)
MIX_MODES_FIGURES = tuple("mix_" + k for k in MODES_FIGURES)
RANK_FIGURES = ("rank_dev", "rank_dev_final", "rank_dev_traj", "rank_mean", "rank_mean_traj", "rank_cov50",
                "rank_nom50", "rank_cov90", "rank_nom90", "rank_degenerate")
FULLCOV_RANK_FIGURES = tuple("fullcov_" + k for k in RANK_FIGURES)
MIX_RANK_FIGURES = tuple("mix_" + k for k in RANK_FIGURES)
KIN_GROUPS = ("speed", "acc", "lacc", "straight")
KIN_FIGURES = tuple(f"kin_{f}_{g}" for f in ("crps", "pit", "dev", "draw", "target") for g in KIN_GROUPS)
FULLCOV_KIN_FIGURES = tuple("fullcov_" + k for k in KIN_FIGURES)
MIX_KIN_FIGURES = tuple("mix_" + k for k in KIN_FIGURES)
CPL_FEATURES = ("min", "fin")
CPL_FIGURES = ("cpl_couples",) + tuple(f"cpl_{f}_{g}" for f in ("crps", "pit", "dev", "draw", "target")
                                       for g in CPL_FEATURES)
FULLCOV_CPL_FIGURES = tuple("fullcov_" + k for k in CPL_FIGURES)
MIX_CPL_FIGURES = tuple("mix_" + k for k in CPL_FIGURES)
SCN_FEATURES = ("typ", "loc", "spr")
SCN_FIGURES = (("scn_frames", "scn_es") + tuple(f"scn_{f}_{g}" for g in SCN_FEATURES for f in ("dev", "pit"))
               + ("scn_draw_loc", "scn_target_loc", "scn_draw_spr", "scn_target_spr"))
FULLCOV_SCN_FIGURES = tuple("fullcov_" + k for k in SCN_FIGURES)
MIX_SCN_FIGURES = tuple("mix_" + k for k in SCN_FIGURES)
COUPLED_SCN_FIGURES = tuple("coupled_" + k for k in SCN_FIGURES)
SMD_FIGURES = ("smd_frames", "smd_jade", "smd_jfde", "smd_brier_jade", "smd_brier_jfde", "smd_miss", "smd_cost",
               "smd_raw_jade", "smd_all_jade", "smd_rounds")
FULLCOV_SMD_FIGURES = tuple("fullcov_" + k for k in SMD_FIGURES)
MIX_SMD_FIGURES = tuple("mix_" + k for k in SMD_FIGURES)
COUPLED_SMD_FIGURES = tuple("coupled_" + k for k in SMD_FIGURES)
COUPLED_FIGURES = ("coupled_share", "coupled_nll", "coupled_nll_gain", "coupled_q_within", "coupled_q_between",
                   "coupled_clipped")
COUPLED_JOINT_FIGURES = ("coupled_jade", "coupled_jfde", "coupled_collision_rate",
                         "coupled_collision_rate_best")
COUPLED_CPL_FIGURES = tuple("coupled_" + k for k in CPL_FIGURES)


def coupled_figures(head, st):
    """COUPLED_FIGURES of a fitted coupled.CoupledHead and its CoupledStats on
    the left-out scenes."""
    return dict(coupled_share=st.share, coupled_nll=st.nll, coupled_nll_gain=st.nll_gain,
                coupled_q_within=st.q_within_ratio, coupled_q_between=st.q_between_ratio,
                coupled_clipped=head.clipped)


def coupled_joint_figures(je):
    """COUPLED_JOINT_FIGURES of a CoupledHead.joint_eval result."""
    return dict(coupled_jade=je.jade, coupled_jfde=je.jfde, coupled_collision_rate=je.collision_rate,
                coupled_collision_rate_best=je.collision_rate_best)


def calib_figures(hs):
    """CALIB_FIGURES of a HeadStats taken at CALIB_LEVELS."""
    cov = hs.coverage_all
    at = {p: float(cov[i]) for i, p in enumerate(hs.levels)}
    return dict(nll=hs.nll, coverage_50=at[0.5], coverage_90=at[0.9], coverage_95=at[0.95],
                ece=hs.ece, q_ratio=hs.q_ratio)


def fullcov_figures(bk, st):
    """FULLCOV_FIGURES of a best-of-K result and a FullCovStats taken at
    CALIB_LEVELS with the same head."""
    at = {p: float(c) for p, c in zip(st.levels, st.coverage_joint)}
    return dict(fullcov_min_ade=bk.min_ade, fullcov_min_fde=bk.min_fde, fullcov_nll=st.nll,
                fullcov_coverage_90=at[0.9], fullcov_q_ratio=st.q_ratio,
                fullcov_lag1_corr=st.lag1_corr)


def fullcov_joint_figures(je):
    """FULLCOV_JOINT_FIGURES of a FullCovHead.joint_eval result (the mean's and
    the ground truth's collision rates do not depend on the head: they are in
    JOINT_FIGURES)."""
    return dict(fullcov_jade=je.jade, fullcov_jfde=je.jfde, fullcov_collision_rate=je.collision_rate,
                fullcov_collision_rate_best=je.collision_rate_best)


def mixture_joint_figures(je):
    """MIX_JOINT_FIGURES of a MixtureHead.joint_eval result."""
    return dict(mix_jade=je.jade, mix_jfde=je.jfde, mix_collision_rate=je.collision_rate,
                mix_collision_rate_best=je.collision_rate_best)


def kde_figures(kd, prefix=""):
    """KDE_FIGURES (``prefix`` "fullcov_": FULLCOV_KDE_FIGURES, "mix_":
    MIX_KDE_FIGURES) of a KdeNll."""
    return {prefix + "kde_nll": kd.kde_nll, prefix + "kde_nll_final": kd.kde_nll_final,
            prefix + "kde_clipped": kd.clipped_share}


def score_figures(sc, prefix=""):
    """SCORE_FIGURES (``prefix`` "fullcov_": FULLCOV_SCORE_FIGURES, "mix_":
    MIX_SCORE_FIGURES) of a scores.SampleScores."""
    return {prefix + k: getattr(sc, k) for k in SCORE_FIGURES}


def _score_line(name, K, dataset, res, prefix=""):
    """The log line of one head's SCORE_FIGURES."""
    v = {k: res[prefix + k] for k in SCORE_FIGURES}
    return (f"{name} of the {K} draws on dataset {dataset}: energy score 24-D "
            f"{v['es_traj']:.6g} ADE {v['es_ade']:.6g} FDE {v['es_fde']:.6g}, expected ADE / FDE of a "
            f"draw {v['mean_ade']:.6g} / {v['mean_fde']:.6g}, APD {v['apd']:.6g}, variogram score "
            f"{v['vs']:.6g}")


def modes_figures(sm, prefix=""):
    """MODES_FIGURES (``prefix`` "fullcov_": FULLCOV_MODES_FIGURES, "mix_":
    MIX_MODES_FIGURES) of a modes.SampleModes, and after them
    ``modes_miss_rate`` when it was taken with a miss radius > 0."""
    fig = {prefix + k: getattr(sm, k[len("modes_"):]) for k in MODES_FIGURES}
    if sm.miss_radius > 0:
        fig[prefix + "modes_miss_rate"] = sm.miss_rate
    return fig


def _modes_line(name, sm, K, dataset, res, prefix=""):
    """The log line of one head's MODES_FIGURES, next to that head's minADE_K."""
    v = {k: res[prefix + k] for k in MODES_FIGURES}
    line = (f"{name} on dataset {dataset}: {sm.modes} centres of {sm.k} draws after {sm.iters} "
            f"iterations, minADE_{sm.modes} {v['modes_min_ade']:.6g} minFDE_{sm.modes} "
            f"{v['modes_min_fde']:.6g} (minADE_{K} / minFDE_{K} of the {K} raw draws "
            f"{res[prefix + 'min_ade']:.6g} / {res[prefix + 'min_fde']:.6g}), Brier "
            f"{v['modes_brier_ade']:.6g} / {v['modes_brier_fde']:.6g}, inertia "
            f"{v['modes_inertia']:.6g}, live centres {v['modes_live']:.4g}")
    if sm.miss_radius > 0:
        line += f", miss rate at {sm.miss_radius:g} {res[prefix + 'modes_miss_rate']:.4f}"
    return line


def rank_figures(sr, prefix=""):
    """RANK_FIGURES (``prefix`` "fullcov_": FULLCOV_RANK_FIGURES, "mix_":
    MIX_RANK_FIGURES) of a ranks.SampleRanks."""
    nom50, cov50 = sr.coverage(0.5)
    nom90, cov90 = sr.coverage(0.9)
    fig = dict(rank_dev=sr.dev, rank_dev_final=sr.dev_final, rank_dev_traj=sr.dev_traj, rank_mean=sr.mean,
               rank_mean_traj=sr.mean_traj, rank_cov50=cov50, rank_nom50=nom50, rank_cov90=cov90,
               rank_nom90=nom90, rank_degenerate=sr.degenerate_share)
    return {prefix + k: fig[k] for k in RANK_FIGURES}


def _rank_line(name, sr, dataset, res, prefix=""):
    """The log line of one head's RANK_FIGURES."""
    v = {k: res[prefix + k] for k in RANK_FIGURES}
    return (f"{name} of the {sr.k} draws on dataset {dataset}: {sr.bins} bins, distance from uniform "
            f"steps {v['rank_dev']:.4f} final step {v['rank_dev_final']:.4f} trajectory "
            f"{v['rank_dev_traj']:.4f}, mean rank steps {v['rank_mean']:.4f} trajectory "
            f"{v['rank_mean_traj']:.4f} (1/2 when calibrated; steps above: too narrow), targets among "
            f"the {v['rank_nom50']:.4f} most typical points {v['rank_cov50']:.4f}, among the "
            f"{v['rank_nom90']:.4f} most typical {v['rank_cov90']:.4f}, degenerate steps "
            f"{v['rank_degenerate']:.4f}")


def kin_figures(sk, prefix=""):
    """KIN_FIGURES (``prefix`` "fullcov_": FULLCOV_KIN_FIGURES, "mix_":
    MIX_KIN_FIGURES) of a kin.SampleKin."""
    fig = {}
    for g in KIN_GROUPS:
        fig.update({f"kin_crps_{g}": sk.crps(g), f"kin_pit_{g}": sk.pit_mean(g), f"kin_dev_{g}": sk.dev(g),
                    f"kin_draw_{g}": sk.draw_mean(g), f"kin_target_{g}": sk.target_mean(g)})
    return {prefix + k: fig[k] for k in KIN_FIGURES}


def _kin_line(name, sk, dataset, res, prefix=""):
    """The log line of one head's KIN_FIGURES."""
    parts = [f"{g} crps {res[prefix + 'kin_crps_' + g]:.4f} pit {res[prefix + 'kin_pit_' + g]:.4f} "
             f"dev {res[prefix + 'kin_dev_' + g]:.4f} draws {res[prefix + 'kin_draw_' + g]:.4f} "
             f"targets {res[prefix + 'kin_target_' + g]:.4f}" for g in KIN_GROUPS]
    return (f"{name} of the {sk.k} draws on dataset {dataset}: {sk.bins} bins (pit 1/2 when calibrated; "
            f"below: the draws' feature is the larger), " + ", ".join(parts))


def couple_figures(cs, prefix=""):
    """CPL_FIGURES (``prefix`` "fullcov_": FULLCOV_CPL_FIGURES, "mix_":
    MIX_CPL_FIGURES) of a couples.CoupleScores."""
    fig = {"cpl_couples": cs.couples}
    for g in CPL_FEATURES:
        fig.update({f"cpl_crps_{g}": cs.crps(g), f"cpl_pit_{g}": cs.pit_mean(g), f"cpl_dev_{g}": cs.dev(g),
                    f"cpl_draw_{g}": cs.draw_mean(g), f"cpl_target_{g}": cs.target_mean(g)})
    return {prefix + k: fig[k] for k in CPL_FIGURES}


def scene_figures(sr, prefix=""):
    """SCN_FIGURES (``prefix`` "fullcov_", "mix_", "coupled_": those heads') of
    a sceneranks.SceneRanks."""
    fig = {"scn_frames": sr.frames, "scn_es": sr.es}
    for g in SCN_FEATURES:
        fig.update({f"scn_dev_{g}": sr.dev(g), f"scn_pit_{g}": sr.pit(g)})
    for g in SCN_FEATURES[1:]:
        fig.update({f"scn_draw_{g}": sr.draw(g), f"scn_target_{g}": sr.target(g)})
    return {prefix + k: fig[k] for k in SCN_FIGURES}


def _scene_line(name, sr, dataset, res, prefix=""):
    """The log line of one head's SCN_FIGURES."""
    parts = [f"{g} dev {res[prefix + 'scn_dev_' + g]:.4f} pit {res[prefix + 'scn_pit_' + g]:.4f}"
             for g in SCN_FEATURES]
    parts += [f"{g} draws {res[prefix + 'scn_draw_' + g]:.4f} targets {res[prefix + 'scn_target_' + g]:.4f}"
              for g in SCN_FEATURES[1:]]
    return (f"{name} of the {sr.k} joint draws on dataset {dataset}: {res[prefix + 'scn_frames']} scenes of "
            f"two pedestrians or more, {sr.bins} bins (pit 1/2 when calibrated; loc near 1 and spr near 0: "
            f"the pedestrians move together more than the draws do), fair energy score "
            f"{res[prefix + 'scn_es']:.6g} (nearly blind to dependence: reported, never gated on), "
            + ", ".join(parts))


def scene_mode_figures(sm, prefix=""):
    """SMD_FIGURES (``prefix`` "fullcov_", "mix_", "coupled_": those heads') of
    a scenemodes.SceneModes."""
    fig = {"smd_frames": sm.frames, "smd_jade": sm.jade, "smd_jfde": sm.jfde, "smd_brier_jade": sm.brier_jade,
           "smd_brier_jfde": sm.brier_jfde, "smd_miss": sm.miss_rate, "smd_cost": sm.cost,
           "smd_raw_jade": sm.raw_jade, "smd_all_jade": sm.all_jade, "smd_rounds": sm.rounds}
    return {prefix + k: fig[k] for k in SMD_FIGURES}


def _scene_mode_line(name, sm, dataset, res, prefix=""):
    """The log line of one head's SMD_FIGURES."""
    v = {k: res[prefix + k] for k in SMD_FIGURES}
    return (f"{name} of the {sm.k} joint draws on dataset {dataset}: {v['smd_frames']} scenes reduced to "
            f"{sm.modes} modes in {v['smd_rounds']:.3g} rounds of at most {sm.iters}, minJADE_{sm.modes} "
            f"{v['smd_jade']:.6g} minJFDE_{sm.modes} {v['smd_jfde']:.6g} (the first {sm.modes} raw draws "
            f"{v['smd_raw_jade']:.6g}, all {sm.k} draws {v['smd_all_jade']:.6g}), Brier "
            f"{v['smd_brier_jade']:.6g} / {v['smd_brier_jfde']:.6g}, cost {v['smd_cost']:.6g}, scene miss "
            f"rate at {sm.miss_radius:g} {v['smd_miss']:.4f}")


def _couple_line(name, cs, dataset, res, prefix=""):
    """The log line of one head's CPL_FIGURES."""
    parts = [f"{g} crps {res[prefix + 'cpl_crps_' + g]:.4f} pit {res[prefix + 'cpl_pit_' + g]:.4f} "
             f"dev {res[prefix + 'cpl_dev_' + g]:.4f} draws {res[prefix + 'cpl_draw_' + g]:.4f} "
             f"targets {res[prefix + 'cpl_target_' + g]:.4f}" for g in CPL_FEATURES]
    return (f"{name} of the {cs.k} joint draws on dataset {dataset}: {res[prefix + 'cpl_couples']} couples "
            f"within reach {cs.reach:g} of {cs.member_couples}, {cs.bins} bins (pit 1/2 when calibrated; "
            f"below: the draws keep the couples further apart), " + ", ".join(parts))


def mixture_figures(mx, bk, st, fit):
    """MIX_FIGURES of a fitted MixtureHead: its best-of-K result and
    MixtureStats on the evaluated scenes, and the MixtureFit that made it
    (``mix_loglik_gain``: the last minus the first log-likelihood per pair over
    the fit)."""
    return dict(mix_min_ade=bk.min_ade, mix_min_fde=bk.min_fde, mix_nll=st.nll,
                mix_components=mx.components, mix_weight_max=float(mx.weights.max().item()),
                mix_loglik_gain=fit.gain)


def left_out_plan(args, nmax):
    """The RealPlan of every distinct scene (2 <= P <= nmax) of the left-out
    dataset; FileNotFoundError when it is not under --data_root (5,
    town_center.csv, is absent from the reference's data)."""
    l = int(args.leaveDataset)
    names = [n for n, i in rd.DATASETS.items() if i == l]
    if not names:
        raise FileNotFoundError(f"dataset {l} is not among the shipped datasets {rd.DATASETS}")
    raw = rd.load_raw(names, args.data_root)
    n = rd.count_scenes(raw, nmax)
    if n == 0:
        raise ValueError(f"dataset {l}: no scene with 2 <= P <= {nmax}")
    return rd.plan_scenes(n, raw, nmax=nmax)


def _fused_step(args, params, plan, device):
    """One fused step over the plan's scenes (F = 1, stride 0) -> (device
    tensors, the step's outputs, n_frames = 1 per scene)."""
    from .train import context_G
    S = plan.S
    t = plan.to_device(device, F=1)
    G = torch.from_numpy(context_G(args.seed, S)).to(device)
    h0 = torch.zeros((S, fs.HIDDEN_LEN, args.rnn_size), device=device)
    one = torch.ones(S, dtype=torch.int32, device=device)
    out = fs.step_fused(params, t["pos"], t["vislet"], G, t["targets"], t["n_active"], h0,
                        n_frames=one, ped_mask=t["ped_mask"], stride=0, lam=args.lambda_param)
    return t, out, one


def fold_plan(args, nmax):
    """The RealPlan of the fold's training datasets, as run_train_mode plans
    them (--train_scenes honoured), at the parameters' Nmax."""
    raw = rd.load_raw(list(rd.fold_datasets(args.leaveDataset)), args.data_root)
    return rd.plan_scenes(args.train_scenes or rd.count_scenes(raw, nmax), raw, nmax=nmax)


def evaluate_best_of_k(args, params, device, log=print, keep=None):
    """--num_samples K on --leaveDataset with ``params`` (a G2KParams on
    ``device``).  Logs and returns {scenes, pairs, K, ade, fde, min_ade,
    min_fde} (errors per (scene, pedestrian) pair; ade / fde: the mean
    prediction's), with --collision_radius R > 0 also JOINT_FIGURES from one
    joint_eval launch and a second log line.  --fit_head train / eval first
    replaces the head by the closed-form fit (GaussianHead.fit) on the fold's
    training scenes / on the left-out scenes themselves; --calibration 1
    (implied by --fit_head) adds CALIB_FIGURES from one stats launch on the
    left-out scenes with the head in use, and a log line.  --fullcov_head
    train / eval then fits a FullCovHead on the same scenes as --fit_head
    would, runs its stats and best_of_k on the left-out scenes and adds
    FULLCOV_FIGURES and a log line, and with --collision_radius R > 0 also
    FULLCOV_JOINT_FIGURES from one FullCovHead.joint_eval launch and one more
    log line (``keep["fullcov"]["joint"]``).  --kde_nll 1 adds KDE_FIGURES
    from one GaussianHead.kde_nll launch (same K and seed, floor --kde_floor)
    and a log line, and with --fullcov_head FULLCOV_KDE_FIGURES from one
    FullCovHead.kde_nll launch and a log line (``keep["kde"]``,
    ``keep["fullcov"]["kde"]``).  --mixture_head train / eval then fits a
    MixtureHead of --mixture_components components by --mixture_iters EM
    iterations on the same scenes as --fullcov_head's modes (started by
    ``MixtureHead.init_from`` a no-head full-covariance stats launch on them),
    runs its stats and best_of_k on the left-out scenes and adds MIX_FIGURES
    and a log line (``keep["mixture"]``); with --collision_radius R > 0 also
    MIX_JOINT_FIGURES from one MixtureHead.joint_eval launch and with
    --kde_nll 1 MIX_KDE_FIGURES from one MixtureHead.kde_nll launch, a log
    line each, after the mixture's line and with the other heads' K, seed,
    radius and floor (``keep["mixture"]["joint"]``, ``keep["mixture"]["kde"]``).
    --sample_scores 1 (2 <= K <= 256) adds SCORE_FIGURES from one
    GaussianHead.sample_scores launch (csrc/g2k_scores.hip; same predictions, K
    and seed) after the per-step head's other figures, and FULLCOV_SCORE_FIGURES
    / MIX_SCORE_FIGURES at the end of those heads' blocks, a log line each
    (``keep["scores"]``, ``keep["fullcov"]["scores"]``,
    ``keep["mixture"]["scores"]``).  --sample_modes M (1..32) adds
    MODES_FIGURES (and ``modes_miss_rate`` with --miss_radius > 0) from one
    GaussianHead.sample_modes launch (csrc/g2k_modes.hip; --modes_draws draws,
    --modes_iters iterations, seed --sample_seed) directly after the per-step
    head's score figures, and FULLCOV_MODES_FIGURES / MIX_MODES_FIGURES after
    those heads' score figures, a log line each that puts minADE_M of the
    centres next to that head's minADE_K (``keep["modes"]``,
    ``keep["fullcov"]["modes"]``, ``keep["mixture"]["modes"]``).
    --sample_ranks 1 (4 <= K <= 255; --rank_bins) adds RANK_FIGURES from one
    GaussianHead.sample_ranks launch (csrc/g2k_ranks.hip; same predictions, K
    and seed) at the end of the per-step head's figures, and
    FULLCOV_RANK_FIGURES / MIX_RANK_FIGURES at the end of those heads' blocks,
    a log line each (``keep["ranks"]``, ``keep["fullcov"]["ranks"]``,
    ``keep["mixture"]["ranks"]``).
    --sample_kinematics 1 (2 <= K <= 255; --kin_bins) adds KIN_FIGURES from one
    GaussianHead.sample_kin launch (csrc/g2k_kin.hip; same predictions, K and
    seed) after the rank figures, and FULLCOV_KIN_FIGURES / MIX_KIN_FIGURES at
    the end of those heads' blocks, a log line each (``keep["kin"]``,
    ``keep["fullcov"]["kin"]``, ``keep["mixture"]["kin"]``).
    --couple_scores 1 (2 <= K <= 64; --couple_bins, --couple_reach) adds
    CPL_FIGURES from one GaussianHead.couple_scores call (csrc/g2k_couples.hip;
    same predictions, K and seed) directly after the kinematic figures, and
    FULLCOV_CPL_FIGURES / MIX_CPL_FIGURES after those heads' kinematic figures,
    a log line each (``keep["couples"]``, ``keep["fullcov"]["couples"]``,
    ``keep["mixture"]["couples"]``).
    --scene_ranks 1 (2 <= K <= 64; --scene_bins) adds SCN_FIGURES directly
    after the same head's couple-distance figures, from one
    ``scene_ranks`` call per head in use (csrc/g2k_scene_ranks.hip), the
    other heads' prefixed "fullcov_" / "mix_" / "coupled_", a log line each
    (``keep["scene_ranks"]``, ``keep[<head>]["scene_ranks"]``).
    --scene_modes M (1..32; max(M, 2) <= K <= 64; --scene_modes_iters,
    --miss_radius) adds SMD_FIGURES directly after the same head's
    scene-rank figures, from one ``scene_modes`` call per head in use
    (csrc/g2k_scene_modes.hip), the other heads' prefixed "fullcov_" / "mix_"
    / "coupled_", a log line each (``keep["scene_modes"]``,
    ``keep[<head>]["scene_modes"]``).
    --coupled_head train / eval then fits the scene-coupled head
    (coupled.CoupledHead, csrc/g2k_coupled.hip: closed form) on the same
    scenes as --fullcov_head's modes and adds COUPLED_FIGURES from one stats
    launch on the left-out scenes and a log line; with --collision_radius R >
    0 also COUPLED_JOINT_FIGURES and with --couple_scores 1
    COUPLED_CPL_FIGURES, one launch and one log line each
    (``keep["coupled"]``).
    ``keep`` (a dict)
    receives the plan, the predictions, the head and the kernels' outputs for
    a caller that checks them."""
    K = int(args.num_samples)
    if K < 1:
        raise ValueError("--num_samples K must be >= 1")
    if getattr(args, "kde_nll", 0) and K < 4:
        raise ValueError("--kde_nll 1 needs --num_samples K >= 4")
    want_scores = bool(getattr(args, "sample_scores", 0))
    if want_scores and not 2 <= K <= 256:
        raise ValueError("--sample_scores 1 needs --num_samples K with 2 <= K <= 256")
    want_ranks = bool(getattr(args, "sample_ranks", 0))
    if want_ranks:
        from . import ranks as rk
        if not rk.KMIN <= K <= rk.KMAX:
            raise ValueError("--sample_ranks 1 needs --num_samples K with 4 <= K <= 255")
        try:
            rank_bins = rk.check_k_bins(K, int(getattr(args, "rank_bins", 0) or 0))[1]
        except ValueError:
            raise ValueError(f"--rank_bins must be 0 (automatic) or a divisor of K + 1 = {K + 1} in "
                             f"1..{rk.BMAX}") from None
        ranks_kw = dict(seed=args.sample_seed, want_per_ped=keep is not None)
    want_kin = bool(getattr(args, "sample_kinematics", 0))
    if want_kin:
        from . import kin as kn
        if not kn.KMIN <= K <= kn.KMAX:
            raise ValueError("--sample_kinematics 1 needs --num_samples K with 2 <= K <= 255")
        try:
            kin_bins = kn.check_k_bins(K, int(getattr(args, "kin_bins", 0) or 0))[1]
        except ValueError:
            raise ValueError(f"--kin_bins must be 0 (automatic) or a divisor of K + 1 = {K + 1} in "
                             f"1..{kn.BMAX}") from None
        kin_kw = dict(seed=args.sample_seed, want_per_ped=keep is not None)
    want_cpl = bool(getattr(args, "couple_scores", 0))
    if want_cpl:
        from . import couples as cp
        if not cp.KMIN <= K <= cp.KMAX:
            raise ValueError("--couple_scores 1 needs --num_samples K with 2 <= K <= 64")
        try:
            cpl_bins = cp.check_k_bins(K, int(getattr(args, "couple_bins", 0) or 0))[1]
        except ValueError:
            raise ValueError(f"--couple_bins must be 0 (automatic) or a divisor of K + 1 = {K + 1} in "
                             f"1..{cp.BMAX}") from None
        cpl_reach = float(getattr(args, "couple_reach", 0.0) or 0.0)
        if not cpl_reach >= 0.0:
            raise ValueError("--couple_reach must be >= 0 (0: every couple)")
        cpl_kw = dict(seed=args.sample_seed, reach=cpl_reach if cpl_reach > 0 else None,
                      want_per_couple=keep is not None, want_per_frame=keep is not None)
    want_scn = bool(getattr(args, "scene_ranks", 0))
    if want_scn:
        from . import sceneranks as sn
        if not sn.KMIN <= K <= sn.KMAX:
            raise ValueError("--scene_ranks 1 needs --num_samples K with 2 <= K <= 64")
        try:
            scn_bins = sn.check_k_bins(K, int(getattr(args, "scene_bins", 0) or 0))[1]
        except ValueError:
            raise ValueError(f"--scene_bins must be 0 (automatic) or a divisor of K + 1 = {K + 1} in "
                             f"1..{sn.BMAX}") from None
        scn_kw = dict(seed=args.sample_seed, want_per_frame=keep is not None)
    n_smd = int(getattr(args, "scene_modes", 0) or 0)
    if n_smd:
        from . import scenemodes as sd
        if not 1 <= n_smd <= sd.MMAX:
            raise ValueError("--scene_modes M: 0 (off) or 1 <= M <= 32")
        if not max(n_smd, sd.KMIN) <= K <= sd.KMAX:
            raise ValueError("--scene_modes M needs --num_samples K with max(M, 2) <= K <= 64")
        smd_iters = int(getattr(args, "scene_modes_iters", 10))
        if not 0 <= smd_iters <= sd.ITERS_MAX:
            raise ValueError("--scene_modes_iters must be in 0..32")
        smd_radius = float(getattr(args, "miss_radius", 0.0) or 0.0)
        if not (np.isfinite(smd_radius) and smd_radius >= 0):
            raise ValueError("--miss_radius must be finite and >= 0")
        smd_kw = dict(iters=smd_iters, miss_radius=smd_radius, seed=args.sample_seed,
                      want_per_frame=keep is not None, want_modes=keep is not None)
    n_modes = int(getattr(args, "sample_modes", 0) or 0)
    if n_modes:
        if not 1 <= n_modes <= 32:
            raise ValueError("--sample_modes M: 0 (off) or 1 <= M <= 32")
        modes_draws = int(getattr(args, "modes_draws", 256))
        if not n_modes <= modes_draws <= 256:
            raise ValueError("--modes_draws must be in M..256 (M = --sample_modes)")
        modes_iters = int(getattr(args, "modes_iters", 10))
        if not 0 <= modes_iters <= 64:
            raise ValueError("--modes_iters must be in 0..64")
        miss_radius = float(getattr(args, "miss_radius", 0.0) or 0.0)
        if not (np.isfinite(miss_radius) and miss_radius >= 0):
            raise ValueError("--miss_radius must be finite and >= 0")
    fit_mode = getattr(args, "fit_head", "off") or "off"
    calibrate = bool(getattr(args, "calibration", 0)) or fit_mode != "off"
    plan = left_out_plan(args, params.nmax)
    S = plan.S
    t, out, one = _fused_step(args, params, plan, device)
    if params.head is not None:
        gh = GaussianHead(device=device)
        gh.head = params.head.contiguous()
        log("best-of-K: the parameters' learned head (nll_head/head)")
    else:
        gh = GaussianHead(log_sigma=args.head_log_sigma, device=device)
        log(f"best-of-K: no head in the parameters, constant log sigma {args.head_log_sigma}")
    fitted = None
    if fit_mode == "train":
        fplan = fold_plan(args, params.nmax)
        ft, fout, fone = _fused_step(args, params, fplan, device)
        fitted = gh.fit(fout.pred, ft["targets"], ft["n_active"], n_frames=fone,
                        ped_mask=ft["ped_mask"])
        log(f"best-of-K: head replaced by the closed-form fit on {fplan.S} scenes of the fold's "
            f"training datasets ({fitted.pairs} pairs)")
    elif fit_mode == "eval":
        fitted = gh.fit(out.pred, t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
        log(f"best-of-K: head replaced by the closed-form fit on the left-out dataset itself "
            f"({fitted.pairs} pairs): in-sample, a bound and not an estimate")
    bk = gh.best_of_k(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed, n_frames=one,
                      ped_mask=t["ped_mask"], want_per_ped=False)
    res = dict(scenes=S, pairs=bk.pairs, K=K, ade=bk.ade, fde=bk.fde, min_ade=bk.min_ade,
               min_fde=bk.min_fde)
    log(f"best-of-{K} on dataset {args.leaveDataset}: {S} scenes, {res['pairs']} pairs, "
        f"ADE {res['ade']:.6g} FDE {res['fde']:.6g} minADE_{K} {res['min_ade']:.6g} "
        f"minFDE_{K} {res['min_fde']:.6g}")
    joint = None
    radius = float(getattr(args, "collision_radius", 0.0) or 0.0)
    if radius > 0:
        joint = gh.joint_eval(out.pred, t["targets"], t["n_active"], K, radius, seed=args.sample_seed,
                              n_frames=one, ped_mask=t["ped_mask"], want_per_frame=keep is not None)
        res.update({k: getattr(joint, k) for k in JOINT_FIGURES})
        log(f"joint best-of-{K} on dataset {args.leaveDataset}: radius {radius:g}, "
            f"{res['ped_pairs']} couples, JADE_{K} {res['jade']:.6g} JFDE_{K} {res['jfde']:.6g} "
            f"collision rate: samples {res['collision_rate']:.6g} mean {res['collision_rate_pred']:.6g} "
            f"best joint sample {res['collision_rate_best']:.6g} "
            f"ground truth {res['collision_rate_gt']:.6g}")
    want_kde = bool(getattr(args, "kde_nll", 0))
    kde_floor = float(getattr(args, "kde_floor", -20.0))
    kde = None
    if want_kde:
        kde = gh.kde_nll(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                         log_floor=kde_floor, n_frames=one, ped_mask=t["ped_mask"],
                         want_per_ped=keep is not None)
        res.update(kde_figures(kde))
        log(f"KDE-NLL of the {K} draws on dataset {args.leaveDataset}: {res['kde_nll']:.6g} per pair "
            f"and step, final step {res['kde_nll_final']:.6g}, floor {kde_floor:g} reached by "
            f"{res['kde_clipped']:.4f} of the steps")
    calib = None
    if calibrate:
        calib = gh.stats(out.pred, t["targets"], t["n_active"], CALIB_LEVELS, n_frames=one,
                         ped_mask=t["ped_mask"])
        res.update(calib_figures(calib))
        sig = torch.exp(gh.head[:2]).cpu().numpy()
        log(f"calibration on dataset {args.leaveDataset}: NLL per pair {res['nll']:.6g}, coverage "
            f"50% {res['coverage_50']:.4f} 90% {res['coverage_90']:.4f} 95% {res['coverage_95']:.4f}, "
            f"ECE {res['ece']:.4f}, q_ratio {res['q_ratio']:.6g}, sigma_x / sigma_y step 1 "
            f"{sig[0, 0]:.6g} / {sig[1, 0]:.6g} step 12 {sig[0, -1]:.6g} / {sig[1, -1]:.6g}")
    scores = None
    if want_scores:
        scores = gh.sample_scores(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                                  n_frames=one, ped_mask=t["ped_mask"], want_per_ped=keep is not None)
        res.update(score_figures(scores))
        log(_score_line("sample scores", K, args.leaveDataset, res))
    modes = None
    if n_modes:
        modes_kw = dict(iters=modes_iters, seed=args.sample_seed, miss_radius=miss_radius, n_frames=one,
                        ped_mask=t["ped_mask"], want_per_ped=keep is not None)
        modes = gh.sample_modes(out.pred, t["targets"], t["n_active"], modes_draws, n_modes, **modes_kw)
        res.update(modes_figures(modes))
        log(_modes_line("sample modes", modes, K, args.leaveDataset, res))
    ranks = None
    if want_ranks:
        ranks = gh.sample_ranks(out.pred, t["targets"], t["n_active"], K, rank_bins, n_frames=one,
                                ped_mask=t["ped_mask"], **ranks_kw)
        res.update(rank_figures(ranks))
        log(_rank_line("sample ranks", ranks, args.leaveDataset, res))
    kin = None
    if want_kin:
        kin = gh.sample_kin(out.pred, t["targets"], t["n_active"], K, kin_bins, n_frames=one,
                            ped_mask=t["ped_mask"], **kin_kw)
        res.update(kin_figures(kin))
        log(_kin_line("sample kinematics", kin, args.leaveDataset, res))
    cpl = None
    if want_cpl:
        cpl = gh.couple_scores(out.pred, t["targets"], t["n_active"], K, cpl_bins, n_frames=one,
                               ped_mask=t["ped_mask"], **cpl_kw)
        res.update(couple_figures(cpl))
        log(_couple_line("couple scores", cpl, args.leaveDataset, res))
    scn = None
    if want_scn:
        scn = gh.scene_ranks(out.pred, t["targets"], t["n_active"], K, scn_bins, n_frames=one,
                             ped_mask=t["ped_mask"], **scn_kw)
        res.update(scene_figures(scn))
        log(_scene_line("scene ranks", scn, args.leaveDataset, res))
    smd = None
    if n_smd:
        smd = gh.scene_modes(out.pred, t["targets"], t["n_active"], K, n_smd, n_frames=one,
                             ped_mask=t["ped_mask"], **smd_kw)
        res.update(scene_mode_figures(smd))
        log(_scene_mode_line("scene modes", smd, args.leaveDataset, res))
    fc_mode = getattr(args, "fullcov_head", "off") or "off"
    fc = fc_st = fc_bk = fc_joint = fc_kde = fc_scores = fc_modes = fc_ranks = fc_kin = fc_cpl = fc_scn = fc_smd = None
    if fc_mode != "off":
        from .fullcov import FullCovHead
        fc = FullCovHead(device=device)
        if fc_mode == "train":
            fplan = fold_plan(args, params.nmax)
            ft, fout, fone = _fused_step(args, params, fplan, device)
            ffit = fc.fit(fout.pred, ft["targets"], ft["n_active"], n_frames=fone,
                          ped_mask=ft["ped_mask"])
            where = f"{fplan.S} scenes of the fold's training datasets ({ffit.pairs} pairs)"
        else:
            ffit = fc.fit(out.pred, t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
            where = (f"the left-out dataset itself ({ffit.pairs} pairs): in-sample, a bound and not "
                     f"an estimate")
        fc_st = fc.stats(out.pred, t["targets"], t["n_active"], CALIB_LEVELS, n_frames=one,
                         ped_mask=t["ped_mask"])
        fc_bk = fc.best_of_k(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                             n_frames=one, ped_mask=t["ped_mask"], want_per_ped=False)
        res.update(fullcov_figures(fc_bk, fc_st))
        log(f"full-covariance head on dataset {args.leaveDataset}: closed-form fit on {where}; "
            f"minADE_{K} {res['fullcov_min_ade']:.6g} minFDE_{K} {res['fullcov_min_fde']:.6g} "
            f"(per-step head {res['min_ade']:.6g} / {res['min_fde']:.6g}), joint NLL per pair "
            f"{res['fullcov_nll']:.6g}, coverage 90% {res['fullcov_coverage_90']:.4f}, q_ratio "
            f"{res['fullcov_q_ratio']:.6g}, lag-1 correlation of the x-residuals "
            f"{res['fullcov_lag1_corr']:.4f} (left-out scenes)")
        if radius > 0:
            fc_joint = fc.joint_eval(out.pred, t["targets"], t["n_active"], K, radius,
                                     seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"],
                                     want_per_frame=keep is not None)
            res.update(fullcov_joint_figures(fc_joint))
            log(f"full-covariance joint best-of-K on dataset {args.leaveDataset}: radius {radius:g}, "
                f"K {K}, JADE_{K} {res['fullcov_jade']:.6g} JFDE_{K} {res['fullcov_jfde']:.6g} "
                f"(per-step head {res['jade']:.6g} / {res['jfde']:.6g}), collision rate: samples "
                f"{res['fullcov_collision_rate']:.6g} (per-step head {res['collision_rate']:.6g}) "
                f"best joint sample {res['fullcov_collision_rate_best']:.6g} (per-step head "
                f"{res['collision_rate_best']:.6g})")
        if want_kde:
            fc_kde = fc.kde_nll(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                                log_floor=kde_floor, n_frames=one, ped_mask=t["ped_mask"],
                                want_per_ped=keep is not None)
            res.update(kde_figures(fc_kde, "fullcov_"))
            log(f"full-covariance KDE-NLL of the {K} draws on dataset {args.leaveDataset}: "
                f"{res['fullcov_kde_nll']:.6g} per pair and step (per-step head "
                f"{res['kde_nll']:.6g}), final step {res['fullcov_kde_nll_final']:.6g} (per-step "
                f"head {res['kde_nll_final']:.6g}), floor {kde_floor:g} reached by "
                f"{res['fullcov_kde_clipped']:.4f} of the steps")
        if want_scores:
            fc_scores = fc.sample_scores(out.pred, t["targets"], t["n_active"], K,
                                         seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"],
                                         want_per_ped=keep is not None)
            res.update(score_figures(fc_scores, "fullcov_"))
            log(_score_line("full-covariance sample scores", K, args.leaveDataset, res, "fullcov_"))
        if n_modes:
            fc_modes = fc.sample_modes(out.pred, t["targets"], t["n_active"], modes_draws, n_modes,
                                       **modes_kw)
            res.update(modes_figures(fc_modes, "fullcov_"))
            log(_modes_line("full-covariance sample modes", fc_modes, K, args.leaveDataset, res,
                            "fullcov_"))
        if want_ranks:
            fc_ranks = fc.sample_ranks(out.pred, t["targets"], t["n_active"], K, rank_bins, n_frames=one,
                                       ped_mask=t["ped_mask"], **ranks_kw)
            res.update(rank_figures(fc_ranks, "fullcov_"))
            log(_rank_line("full-covariance sample ranks", fc_ranks, args.leaveDataset, res, "fullcov_"))
        if want_kin:
            fc_kin = fc.sample_kin(out.pred, t["targets"], t["n_active"], K, kin_bins, n_frames=one,
                                   ped_mask=t["ped_mask"], **kin_kw)
            res.update(kin_figures(fc_kin, "fullcov_"))
            log(_kin_line("full-covariance sample kinematics", fc_kin, args.leaveDataset, res, "fullcov_"))
        if want_cpl:
            fc_cpl = fc.couple_scores(out.pred, t["targets"], t["n_active"], K, cpl_bins, n_frames=one,
                                      ped_mask=t["ped_mask"], **cpl_kw)
            res.update(couple_figures(fc_cpl, "fullcov_"))
            log(_couple_line("full-covariance couple scores", fc_cpl, args.leaveDataset, res, "fullcov_"))
        if want_scn:
            fc_scn = fc.scene_ranks(out.pred, t["targets"], t["n_active"], K, scn_bins, n_frames=one,
                                    ped_mask=t["ped_mask"], **scn_kw)
            res.update(scene_figures(fc_scn, "fullcov_"))
            log(_scene_line("full-covariance scene ranks", fc_scn, args.leaveDataset, res, "fullcov_"))
        if n_smd:
            fc_smd = fc.scene_modes(out.pred, t["targets"], t["n_active"], K, n_smd, n_frames=one,
                                    ped_mask=t["ped_mask"], **smd_kw)
            res.update(scene_mode_figures(fc_smd, "fullcov_"))
            log(_scene_mode_line("full-covariance scene modes", fc_smd, args.leaveDataset, res, "fullcov_"))
    mx_mode = getattr(args, "mixture_head", "off") or "off"
    mx = mx_fit = mx_st = mx_bk = mx_joint = mx_kde = mx_scores = mx_modes = mx_ranks = mx_kin = mx_cpl = mx_scn = mx_smd = None
    if mx_mode != "off":
        from .mixture import MixtureHead
        mx = MixtureHead(components=int(getattr(args, "mixture_components", 3)), device=device)
        iters = int(getattr(args, "mixture_iters", 30))
        if mx_mode == "train":
            fplan = fold_plan(args, params.nmax)
            ft, fout, fone = _fused_step(args, params, fplan, device)
            mx_fit = mx.fit(fout.pred, ft["targets"], ft["n_active"], iters=iters, n_frames=fone,
                            ped_mask=ft["ped_mask"])
            where = f"{fplan.S} scenes of the fold's training datasets ({mx_fit.pairs} pairs)"
        else:
            mx_fit = mx.fit(out.pred, t["targets"], t["n_active"], iters=iters, n_frames=one,
                            ped_mask=t["ped_mask"])
            where = (f"the left-out dataset itself ({mx_fit.pairs} pairs): in-sample, a bound and not "
                     f"an estimate")
        mx_st = mx.stats(out.pred, t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
        mx_bk = mx.best_of_k(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                             n_frames=one, ped_mask=t["ped_mask"], want_per_ped=False)
        res.update(mixture_figures(mx, mx_bk, mx_st, mx_fit))
        log(f"mixture head on dataset {args.leaveDataset}: {iters} EM iterations on {where}; "
            f"{res['mix_components']} live components, largest weight {res['mix_weight_max']:.4f}, "
            f"log-likelihood gained {res['mix_loglik_gain']:.6g} per pair; minADE_{K} "
            f"{res['mix_min_ade']:.6g} minFDE_{K} {res['mix_min_fde']:.6g} (per-step head "
            f"{res['min_ade']:.6g} / {res['min_fde']:.6g}), NLL per pair {res['mix_nll']:.6g} "
            f"(left-out scenes)")
        if radius > 0:
            mx_joint = mx.joint_eval(out.pred, t["targets"], t["n_active"], K, radius,
                                     seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"],
                                     want_per_frame=keep is not None)
            res.update(mixture_joint_figures(mx_joint))
            log(f"mixture joint best-of-K on dataset {args.leaveDataset}: radius {radius:g}, "
                f"K {K}, JADE_{K} {res['mix_jade']:.6g} JFDE_{K} {res['mix_jfde']:.6g} "
                f"(per-step head {res['jade']:.6g} / {res['jfde']:.6g}), collision rate: samples "
                f"{res['mix_collision_rate']:.6g} (per-step head {res['collision_rate']:.6g}) "
                f"best joint sample {res['mix_collision_rate_best']:.6g} (per-step head "
                f"{res['collision_rate_best']:.6g})")
        if want_kde:
            mx_kde = mx.kde_nll(out.pred, t["targets"], t["n_active"], K, seed=args.sample_seed,
                                log_floor=kde_floor, n_frames=one, ped_mask=t["ped_mask"],
                                want_per_ped=keep is not None)
            res.update(kde_figures(mx_kde, "mix_"))
            log(f"mixture KDE-NLL of the {K} draws on dataset {args.leaveDataset}: "
                f"{res['mix_kde_nll']:.6g} per pair and step (per-step head "
                f"{res['kde_nll']:.6g}), final step {res['mix_kde_nll_final']:.6g} (per-step "
                f"head {res['kde_nll_final']:.6g}), floor {kde_floor:g} reached by "
                f"{res['mix_kde_clipped']:.4f} of the steps")
        if want_scores:
            mx_scores = mx.sample_scores(out.pred, t["targets"], t["n_active"], K,
                                         seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"],
                                         want_per_ped=keep is not None)
            res.update(score_figures(mx_scores, "mix_"))
            log(_score_line("mixture sample scores", K, args.leaveDataset, res, "mix_"))
        if n_modes:
            mx_modes = mx.sample_modes(out.pred, t["targets"], t["n_active"], modes_draws, n_modes,
                                       **modes_kw)
            res.update(modes_figures(mx_modes, "mix_"))
            log(_modes_line("mixture sample modes", mx_modes, K, args.leaveDataset, res, "mix_"))
        if want_ranks:
            mx_ranks = mx.sample_ranks(out.pred, t["targets"], t["n_active"], K, rank_bins, n_frames=one,
                                       ped_mask=t["ped_mask"], **ranks_kw)
            res.update(rank_figures(mx_ranks, "mix_"))
            log(_rank_line("mixture sample ranks", mx_ranks, args.leaveDataset, res, "mix_"))
        if want_kin:
            mx_kin = mx.sample_kin(out.pred, t["targets"], t["n_active"], K, kin_bins, n_frames=one,
                                   ped_mask=t["ped_mask"], **kin_kw)
            res.update(kin_figures(mx_kin, "mix_"))
            log(_kin_line("mixture sample kinematics", mx_kin, args.leaveDataset, res, "mix_"))
        if want_cpl:
            mx_cpl = mx.couple_scores(out.pred, t["targets"], t["n_active"], K, cpl_bins, n_frames=one,
                                      ped_mask=t["ped_mask"], **cpl_kw)
            res.update(couple_figures(mx_cpl, "mix_"))
            log(_couple_line("mixture couple scores", mx_cpl, args.leaveDataset, res, "mix_"))
        if want_scn:
            mx_scn = mx.scene_ranks(out.pred, t["targets"], t["n_active"], K, scn_bins, n_frames=one,
                                    ped_mask=t["ped_mask"], **scn_kw)
            res.update(scene_figures(mx_scn, "mix_"))
            log(_scene_line("mixture scene ranks", mx_scn, args.leaveDataset, res, "mix_"))
        if n_smd:
            mx_smd = mx.scene_modes(out.pred, t["targets"], t["n_active"], K, n_smd, n_frames=one,
                                    ped_mask=t["ped_mask"], **smd_kw)
            res.update(scene_mode_figures(mx_smd, "mix_"))
            log(_scene_mode_line("mixture scene modes", mx_smd, args.leaveDataset, res, "mix_"))
    co_mode = getattr(args, "coupled_head", "off") or "off"
    co = co_fit = co_st = co_joint = co_cpl = co_scn = co_smd = None
    if co_mode != "off":
        from .coupled import CoupledHead
        co = CoupledHead(device=device)
        if co_mode == "train":
            fplan = fold_plan(args, params.nmax)
            ft, fout, fone = _fused_step(args, params, fplan, device)
            co_fit = co.fit(fout.pred, ft["targets"], ft["n_active"], n_frames=fone, ped_mask=ft["ped_mask"])
            where = (f"{fplan.S} scenes of the fold's training datasets ({co_fit.pairs} pairs in "
                     f"{co_fit.groups} scene-frames)")
        else:
            co_fit = co.fit(out.pred, t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
            where = (f"the left-out dataset itself ({co_fit.pairs} pairs in {co_fit.groups} scene-frames): "
                     f"in-sample, a bound and not an estimate")
        co_st = co.stats(out.pred, t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
        res.update(coupled_figures(co, co_st))
        log(f"coupled head on dataset {args.leaveDataset}: closed-form fit on {where}, "
            f"{res['coupled_clipped']} eigenvalues clipped; shared part of the residual variance "
            f"{res['coupled_share']:.4f}, joint NLL per pair {res['coupled_nll']:.6g}, "
            f"{res['coupled_nll_gain']:.6g} nats below the independent head with the same marginals, "
            f"q_within {res['coupled_q_within']:.6g} q_between {res['coupled_q_between']:.6g} (1 when "
            f"calibrated; left-out scenes)")
        if radius > 0:
            co_joint = co.joint_eval(out.pred, t["targets"], t["n_active"], K, radius, seed=args.sample_seed,
                                     n_frames=one, ped_mask=t["ped_mask"], want_per_frame=keep is not None)
            res.update(coupled_joint_figures(co_joint))
            log(f"coupled joint best-of-K on dataset {args.leaveDataset}: radius {radius:g}, "
                f"K {K}, JADE_{K} {res['coupled_jade']:.6g} JFDE_{K} {res['coupled_jfde']:.6g} "
                f"(per-step head {res['jade']:.6g} / {res['jfde']:.6g}), collision rate: samples "
                f"{res['coupled_collision_rate']:.6g} (per-step head {res['collision_rate']:.6g}) "
                f"best joint sample {res['coupled_collision_rate_best']:.6g} (per-step head "
                f"{res['collision_rate_best']:.6g})")
        if want_cpl:
            co_cpl = co.couple_scores(out.pred, t["targets"], t["n_active"], K, cpl_bins, n_frames=one,
                                      ped_mask=t["ped_mask"], **cpl_kw)
            res.update(couple_figures(co_cpl, "coupled_"))
            log(_couple_line("coupled couple scores", co_cpl, args.leaveDataset, res, "coupled_"))
        if want_scn:
            co_scn = co.scene_ranks(out.pred, t["targets"], t["n_active"], K, scn_bins, n_frames=one,
                                    ped_mask=t["ped_mask"], **scn_kw)
            res.update(scene_figures(co_scn, "coupled_"))
            log(_scene_line("coupled scene ranks", co_scn, args.leaveDataset, res, "coupled_"))
        if n_smd:
            co_smd = co.scene_modes(out.pred, t["targets"], t["n_active"], K, n_smd, n_frames=one,
                                    ped_mask=t["ped_mask"], **smd_kw)
            res.update(scene_mode_figures(co_smd, "coupled_"))
            log(_scene_mode_line("coupled scene modes", co_smd, args.leaveDataset, res, "coupled_"))
    if keep is not None:
        if co is not None:
            keep.update(coupled=dict(head=co, fit=co_fit, stats=co_st))
            if co_joint is not None:
                keep["coupled"]["joint"] = co_joint
            if co_cpl is not None:
                keep["coupled"]["couples"] = co_cpl
            if co_scn is not None:
                keep["coupled"]["scene_ranks"] = co_scn
            if co_smd is not None:
                keep["coupled"]["scene_modes"] = co_smd
        keep.update(plan=plan, pred=out.pred, head=gh.head, out=bk, n_frames=np.ones(S, np.int32),
                    joint=joint)
        if mx is not None:
            keep.update(mixture=dict(head=mx, fit=mx_fit, stats=mx_st, out=mx_bk))
            if mx_joint is not None:
                keep["mixture"]["joint"] = mx_joint
            if mx_kde is not None:
                keep["mixture"]["kde"] = mx_kde
            if mx_scores is not None:
                keep["mixture"]["scores"] = mx_scores
            if mx_modes is not None:
                keep["mixture"]["modes"] = mx_modes
            if mx_ranks is not None:
                keep["mixture"]["ranks"] = mx_ranks
            if mx_kin is not None:
                keep["mixture"]["kin"] = mx_kin
            if mx_cpl is not None:
                keep["mixture"]["couples"] = mx_cpl
            if mx_scn is not None:
                keep["mixture"]["scene_ranks"] = mx_scn
            if mx_smd is not None:
                keep["mixture"]["scene_modes"] = mx_smd
        if calibrate:
            keep.update(calib=calib, fitted=fitted)
        if kde is not None:
            keep.update(kde=kde)
        if scores is not None:
            keep.update(scores=scores)
        if modes is not None:
            keep.update(modes=modes)
        if ranks is not None:
            keep.update(ranks=ranks)
        if kin is not None:
            keep.update(kin=kin)
        if cpl is not None:
            keep.update(couples=cpl)
        if scn is not None:
            keep.update(scene_ranks=scn)
        if smd is not None:
            keep.update(scene_modes=smd)
        if fc is not None:
            keep.update(fullcov=dict(stats=fc_st, out=fc_bk, fitted=ffit), fullcov_chol=fc.chol)
            if fc_joint is not None:
                keep["fullcov"]["joint"] = fc_joint
            if fc_kde is not None:
                keep["fullcov"]["kde"] = fc_kde
            if fc_scores is not None:
                keep["fullcov"]["scores"] = fc_scores
            if fc_modes is not None:
                keep["fullcov"]["modes"] = fc_modes
            if fc_ranks is not None:
                keep["fullcov"]["ranks"] = fc_ranks
            if fc_kin is not None:
                keep["fullcov"]["kin"] = fc_kin
            if fc_cpl is not None:
                keep["fullcov"]["couples"] = fc_cpl
            if fc_scn is not None:
                keep["fullcov"]["scene_ranks"] = fc_scn
            if fc_smd is not None:
                keep["fullcov"]["scene_modes"] = fc_smd
    return res


def main(argv=None, log=print):
    from .argParser import ArgsParser
    args = ArgsParser().parser.parse_args(argv)
    if args.num_samples < 1:
        raise SystemExit("evaluate: --num_samples K (>= 1) is required")
    prefix = checkpoint.read_state(args.save_dir) if args.save_dir else None
    if not prefix:
        raise SystemExit(f"evaluate: no checkpoint state under --save_dir {args.save_dir!r}")
    device = torch.device(args.device)
    params = checkpoint.load_params(prefix, device=device)
    log(f"evaluate: {prefix} (Nmax {params.nmax})")
    try:
        return evaluate_best_of_k(args, params, device, log=log)
    except FileNotFoundError as exc:
        log(f"evaluation dataset {args.leaveDataset}: {exc}")
        return None


if __name__ == '__main__':
    main()
