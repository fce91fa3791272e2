"""Drop-in replacements for the MVAR / DTF functions of the reference's `src/mtmvar.py`.

Same names, parameters, defaults, return shapes, printed messages and error behaviour as
/root/reference/src/mtmvar.py:35-284 and :551-601; the arithmetic runs on the MI355X through
libhypermvar.so (see `engine.py`).  NumPy arrays in, freshly allocated NumPy arrays out.

Differences that are deliberate and documented in DESIGN.md:
  * `count_corr(..., iwhat=2)` (never used by the reference, quirk Q8) is not provided;
  * `mvar_criterion` gets all orders 1..pmax from ONE factorisation at pmax (the block LDL^T partial
    sums are exactly the lower-order residual covariances) instead of pmax separate fits;
  * `multivariate_spectra` and `full_freq_dtf` share nothing in the reference (each refits the model);
    here each call still fits once, but `mvar_analysis()` returns both from a single fit.
Supported sizes: 1..64 channels, model order 1..32.

FAD (frequency-amplitude-damping) decomposition, mtmvar.py:607-845: `fad_decomposition` and `fad_components_table`
with the reference's signatures, plus `fad_decomposition_batch` for many series in one pass (the fit, the roots and
the residues run on the GPU; see DESIGN.md "FAD").
"""
from __future__ import annotations

import numpy as np
import torch

from .engine import Engine, SingularMatrixError, default_engine

__all__ = ["count_corr", "ar_coeff", "mvar_transfer_function", "multivariate_spectra", "dtf_multivariate",
           "full_freq_dtf", "mvar_criterion", "mvar_analysis", "lag_covariances", "compute_and_plot_mvar",
           "mvar_plot", "fad_decomposition", "fad_decomposition_batch", "fad_components_table", "mvar_residuals",
           "mvar_whiteness", "block_granger_causality"]


# ----------------------------------------------------------------------------- internals
def _as_trials(data, eng: Engine):
    """(m, n) or (m, n, trials) ndarray -> device tensor (trials, m, n)."""
    data = np.asarray(data, dtype=np.float64)
    if data.ndim == 2:
        data = data[:, :, None]
    if data.ndim != 3:
        raise ValueError("signals must have shape (channels, samples) or (channels, samples, trials)")
    x = torch.as_tensor(np.ascontiguousarray(data.transpose(2, 0, 1))).to(eng.device)
    return x


def _lagcov_mean(data, p: int, eng: Engine):
    """Trial-averaged lag covariances in MP layout: (1, p+1, MP, MP).  mtmvar.py:54-85."""
    x = _as_trials(data, eng)
    trials, m, n = x.shape
    if n <= p:
        raise ValueError(f"need more samples ({n}) than the model order ({p})")
    rec = torch.arange(trials, dtype=torch.int64, device=eng.device)
    start = torch.zeros(trials, dtype=torch.int64, device=eng.device)
    R = eng.lagcov(x, rec, start, n, p)
    if trials > 1:
        R = eng.trial_mean(R, m)                          # mtmvar.py:78-85
    return R, m, n


def _fit(data, p: int, eng: Engine, want_logdet=False):
    R, m, n = _lagcov_mean(data, p, eng)
    ar, V, logdet, info = eng.yw_solve(R, m, want_logdet)
    eng.raise_on_info(info, "ar_coeff")
    return ar, V, logdet, m, n


def _order(signals, max_model_order, optimal_model_order, crit_type, plot, comment, style):
    if optimal_model_order is None:
        _, _, optimal_model_order = mvar_criterion(signals, max_model_order, crit_type, plot)
        if style == "spectra":
            print('Optimal model order for all channels: p = ', str(optimal_model_order))
        else:
            comment_str = '' if comment is None else comment + ' '
            print(f'Optimal model order for all {comment_str}channels: p = {optimal_model_order}')
    else:
        if style == "spectra":
            print('Using provided model order: p = ', str(optimal_model_order))
        else:
            print(f'Using provided model order: p = {optimal_model_order}')
    return int(optimal_model_order)


# ----------------------------------------------------------------------------- public API
def lag_covariances(x, p, engine: Engine | None = None):
    """R_l = X[:, :n-l] X[:, l:].T / n, l = 0..p, trial-averaged; (p+1, m, m).  (mtmvar.py:57-59,72-73)"""
    eng = engine or default_engine()
    R, m, _ = _lagcov_mean(x, int(p), eng)
    return R[0, :, :m, :m].cpu().numpy()


def count_corr(x, ip, iwhat):
    """Block-Toeplitz normal equations (mtmvar.py:35-87): returns (r_left, r_right, r)."""
    if iwhat != 1:
        raise NotImplementedError("only the biased estimator (iwhat=1) is implemented (the reference never uses 2)")
    R = lag_covariances(x, ip)
    m = R.shape[1]
    r_left = np.zeros((m * ip, m * ip))
    r_right = np.zeros((m * ip, m))
    for a in range(ip):
        r_right[a * m:(a + 1) * m] = R[a + 1]
        for b in range(ip):
            r_left[a * m:(a + 1) * m, b * m:(b + 1) * m] = R[a - b] if a >= b else R[b - a].T
    return r_left, r_right, R[0].copy()


def ar_coeff(data, model_order=5):
    """MVAR coefficients (channels, channels, model_order) and residual covariance (mtmvar.py:90-123)."""
    eng = default_engine()
    ar, V, _, m, _ = _fit(data, int(model_order), eng)
    return ar[0, :m, :m, :].cpu().numpy(), V[0, :m, :m].cpu().numpy()


def mvar_transfer_function(ar_coeffs, freqs, fs):
    """H(f) = inv(I - sum_k A_k exp(-2 pi i f k / fs)) and A(f); both (chan, chan, len(freqs)) complex.

    mtmvar.py:126-162.  Raises numpy.linalg.LinAlgError('Singular matrix') like np.linalg.inv.
    """
    eng = default_engine()
    ar_coeffs = np.asarray(ar_coeffs, dtype=np.float64)
    m, _, p = ar_coeffs.shape
    mp = eng.pad(m)
    arp = torch.zeros(1, mp, mp, p, dtype=torch.float64, device=eng.device)
    arp[0, :m, :m, :] = torch.as_tensor(ar_coeffs).to(eng.device)
    tw = eng.twiddles(freqs, fs, p)
    out = eng.transfer(arp, m, tw, want_P=False, want_H=True, want_A=True)
    eng.raise_on_info(out["info"], "mvar_transfer_function (inverse of A(f))", per_item=len(np.atleast_1d(freqs)))
    H = eng.to_mmf_complex(out["H"], m)[0].cpu().numpy()
    A = eng.to_mmf_complex(out["A"], m)[0].cpu().numpy()
    return H, A


def mvar_analysis(signals, freqs, fs, model_order, want=("ffdtf", "spectra"), engine: Engine | None = None):
    """One fit, several products: any of 'ar', 'V', 'H', 'A', 'dtf', 'ffdtf', 'spectra', 'pcoh', 'ddtf', 'gpdc'
    as a dict.  `engine`: run on this Engine instead of the process-wide default (extra keyword, not in the reference).

    Not in the reference (which refits for every product, mtmvar.py:165-284); this is what the pipeline
    mirror uses so that ffDTF and spectra share the lag covariances, the solve and the inverses.
    """
    eng = engine or default_engine()
    p = int(model_order)
    ar, V, _, m, _ = _fit(signals, p, eng)
    tw = eng.twiddles(freqs, fs, p)
    need_S = any(k in want for k in ("spectra", "pcoh", "ddtf"))
    need_H = ("H" in want) or need_S
    need_P = any(k in want for k in ("dtf", "ffdtf", "ddtf"))
    t = eng.transfer(ar, m, tw, want_P=need_P, want_H=need_H, want_A=any(k in want for k in ("A", "gpdc")))
    eng.raise_on_info(t["info"], "mvar_transfer_function (inverse of A(f))", per_item=len(np.atleast_1d(freqs)))
    res = {}
    if "ar" in want:
        res["ar"] = ar[0, :m, :m, :].cpu().numpy()
    if "V" in want:
        res["V"] = V[0, :m, :m].cpu().numpy()
    if "H" in want:
        res["H"] = eng.to_mmf_complex(t["H"], m)[0].cpu().numpy()
    if "A" in want:
        res["A"] = eng.to_mmf_complex(t["A"], m)[0].cpu().numpy()
    if "dtf" in want:
        res["dtf"] = eng.normalise(t["P"], t["rowsum"], m, normalise=False)[0][0].cpu().numpy()
    ff = None
    if "ffdtf" in want or "ddtf" in want:
        ff = eng.normalise(t["P"], t["rowsum"], m, normalise=True)[0]
    if "ffdtf" in want:
        res["ffdtf"] = ff[0].cpu().numpy()
    if need_S:
        S = eng.spectra(t["H"], V, m)
        if "spectra" in want:
            res["spectra"] = eng.to_mmf_complex(S, m)[0].cpu().numpy()
        if "pcoh" in want or "ddtf" in want:
            kappa, info = eng.partial_coherence(S, m)
            eng.raise_on_info(info, "partial_coherence")
            if "pcoh" in want:
                res["pcoh"] = kappa[0].cpu().numpy()
            if "ddtf" in want:
                res["ddtf"] = eng.ddtf(ff, kappa)[0].cpu().numpy()
    if "gpdc" in want:
        res["gpdc"] = eng.gpdc(t["A"], V, m)[0].cpu().numpy()
    return res


def multivariate_spectra(signals, freqs, fs, max_model_order=20, optimal_model_order=None, crit_type='AIC'):
    """S(f) = H V H.T (plain transpose, mtmvar.py:199); (N_chan, N_chan, N_f) complex128."""
    p = _order(signals, max_model_order, optimal_model_order, crit_type, True, None, "spectra")
    return mvar_analysis(signals, np.asarray(freqs), fs, p, want=("spectra",))["spectra"]


def dtf_multivariate(signals, freqs, fs, max_model_order=20, optimal_model_order=None, crit_type='AIC', comment=None):
    """Un-normalised |H|^2 (mtmvar.py:204-234, quirk Q2); (N_chan, N_chan, N_f) float64."""
    p = _order(signals, max_model_order, optimal_model_order, crit_type, False, comment, "dtf")
    return mvar_analysis(signals, np.asarray(freqs), fs, p, want=("dtf",))["dtf"]


def full_freq_dtf(signals, freqs, fs, max_model_order=20, optimal_model_order=None, crit_type='AIC'):
    """ffDTF_ij(f) = |H_ij(f)|^2 / sum_f sum_k |H_ik(f)|^2 (mtmvar.py:237-284)."""
    p = _order(signals, max_model_order, optimal_model_order, crit_type, False, None, "dtf")
    return mvar_analysis(signals, np.asarray(freqs), fs, p, want=("ffdtf",))["ffdtf"]


def partial_coherence(spectra):
    """kappa_ij = M_ij / sqrt(M_ii M_jj) with M the minors of the spectral matrix (mtmvar.py:287-338), computed
    from the inverse: M_ij = (-1)^(i+j) det(S) (S^-1)_ji.  (N_chan, N_chan, N_f) complex128 in and out."""
    import torch
    eng = default_engine()
    S = np.ascontiguousarray(np.asarray(spectra, dtype=np.complex128))
    n_chan = S.shape[0]
    if S.ndim != 3 or S.shape[1] != n_chan:
        raise ValueError("spectra must have shape (N_chan, N_chan, N_f)")
    eng.pad(n_chan)
    Sk = eng.pack_complex(torch.from_numpy(S)[None].to(eng.device))
    kappa, info = eng.partial_coherence(Sk, n_chan)
    eng.raise_on_info(info, "partial_coherence")
    return kappa[0].cpu().numpy()


def direct_dtf(signals, freqs, fs, max_model_order=20, optimal_model_order=None, crit_type='AIC'):
    """dDTF = ffDTF * |partial coherence| (mtmvar.py:341-385); one fit instead of the reference's two."""
    p = _order(signals, max_model_order, optimal_model_order, crit_type, True, None, "spectra")
    _order(signals, max_model_order, p if optimal_model_order is None else optimal_model_order, crit_type, False,
           None, "dtf")
    return mvar_analysis(signals, np.asarray(freqs), fs, p, want=("ddtf",))["ddtf"]


def gen_partial_directed_coherence(signals, freqs, fs, max_model_order=20, optimal_model_order=None,
                                   crit_type='AIC'):
    """GPDC_ij(f) = |A_ij|/sigma_i / sqrt(sum_k |A_kj|^2/sigma_k^2) (mtmvar.py:388-468)."""
    p = _order(signals, max_model_order, optimal_model_order, crit_type, False, None, "spectra")
    return mvar_analysis(signals, np.asarray(freqs), fs, p, want=("gpdc",))["gpdc"]


def mvar_criterion(data, max_model_order, crit_type='AIC', plot=False, engine: Engine | None = None):
    """AIC / HQ / SC over p = 1..max_model_order (mtmvar.py:551-601): (crit, p_range, optimal_order)."""
    data = np.asarray(data, dtype=np.float64)
    n_channels, n_samples = data.shape                       # 2-D only, like the reference
    model_order_range = np.arange(1, max_model_order + 1, dtype=int)
    if crit_type == 'AIC':
        pen = 2 * model_order_range * n_channels ** 2 / n_samples
    elif crit_type == 'HQ':
        pen = 2 * np.log(np.log(n_samples)) * model_order_range * n_channels ** 2 / n_samples
    elif crit_type == 'SC':
        pen = np.log(n_samples) * model_order_range * n_channels ** 2 / n_samples
    else:
        raise ValueError("Invalid criterion type. Choose from 'AIC', 'HQ', 'SC'.")
    eng = engine or default_engine()
    _, _, logdet, _, _ = _fit(data, int(max_model_order), eng, want_logdet=True)
    crit = logdet[0].cpu().numpy() + pen
    best = int(np.argmin(crit))                     # first minimum, like the reference's argmin (Q7)
    p_opt = model_order_range[best]
    if plot:
        _criterion_figure(model_order_range, crit, best, crit_type)
    return crit, model_order_range, p_opt


def _one_window(signals, who):
    signals = np.asarray(signals, dtype=np.float64)
    if signals.ndim != 2:
        raise ValueError(f"{who}: signals must have shape (channels, samples); trials are not offered here")
    return signals


def mvar_residuals(signals, model_order):
    """Residuals of the order-`model_order` Yule-Walker fit of one window signals (channels, samples):
    E = X[:, p:] - sum_k A_k X[:, p-k : n-k], shape (channels, samples - model_order), with A_k = ar_coeff(signals,
    model_order)[0][:, :, k-1].  Beyond the reference, which stops at the residual covariance (mtmvar.py:119)."""
    signals = _one_window(signals, "mvar_residuals")
    eng = default_engine()
    p = int(model_order)
    ar, _, _, m, n = _fit(signals, p, eng)
    x = _as_trials(signals, eng)
    zero = torch.zeros(1, dtype=torch.int64, device=eng.device)
    return eng.residuals(x, zero, zero, n, ar)[0].cpu().numpy()


def mvar_whiteness(signals, max_lag, max_model_order=20, optimal_model_order=None, crit_type='AIC'):
    """Residual whiteness of one window's MVAR model (Luetkepohl 2005, section 4.4.3; Hosking 1980; Li & McLeod 1981).
    signals (channels, samples); the order is `optimal_model_order`, or with None the one `mvar_criterion(signals,
    max_model_order, crit_type)` selects.  Returns a dict: model_order, q and p_value (3: Box-Pierce, Li-McLeod, Hosking),
    df = m^2 (max_lag - model_order), q_channel and p_channel (m: per-channel Ljung-Box), acf_fraction (share of the
    residual correlations r_l[i,j], l = 1..max_lag, beyond 1.96 / sqrt(N)), s (max_lag: the per-lag terms) and resid_cov
    (m, m).  Raises LinAlgError('Singular matrix') where the fit or the residual covariance is singular.  The chi-square
    approximation needs samples >> channels^2 max_lag."""
    from .sliding import validation_p_values
    signals = _one_window(signals, "mvar_whiteness")
    eng = default_engine()
    if optimal_model_order is None:
        _, _, optimal_model_order = mvar_criterion(signals, max_model_order, crit_type)
    p = int(optimal_model_order)
    ar, _, _, m, n = _fit(signals, p, eng)
    x = _as_trials(signals, eng)
    zero = torch.zeros(1, dtype=torch.int64, device=eng.device)
    res = eng.model_validation(x, zero, zero, n, ar, max_lag)
    eng.raise_on_info(res["info"], "mvar_whiteness (Cholesky of the residual covariance)")
    h = int(max_lag)
    out = {"model_order": p, "q": res["q"][0].cpu().numpy(), "q_channel": res["q_channel"][0].cpu().numpy(),
           "s": res["s"][0].cpu().numpy(), "resid_cov": res["resid_cov"][0].cpu().numpy(),
           "acf_fraction": float(res["acf_count"][0].item()) / float(h * m * m)}
    df, out["p_value"], out["p_channel"] = validation_p_values(out["q"], out["q_channel"], np.asarray(p), m, h)
    out["df"] = int(df)
    return out


def _criterion_figure(orders, crit, best, crit_type):
    """The figure `mvar_criterion(..., plot=True)` pops up: criterion against model order, the minimum marked."""
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    ax.plot(orders, crit, "o-")
    ax.plot([orders[best]], [crit[best]], "ro")
    ax.set(xlabel="Model order p", ylabel=f"{crit_type} criterion",
           title=f"MVAR Model Order Selection ({crit_type}). The best order = {orders[best]}")
    ax.grid(True)
    plt.show()
    return fig


def mvar_plot(spectra, ff_dtf, freqs, chan_names=None, top_title=""):
    """Minimal m x m grid (|S_ii| on the diagonal, ffDTF j -> i elsewhere); own code, matplotlib only."""
    import matplotlib.pyplot as plt
    m = ff_dtf.shape[0]
    names = list(chan_names) if chan_names is not None else [str(k) for k in range(m)]
    fig, axs = plt.subplots(m, m, figsize=(10, 10), squeeze=False)
    top = float(ff_dtf[~np.eye(m, dtype=bool)].max()) if m > 1 else 1.0
    for i in range(m):
        for j in range(m):
            ax = axs[i, j]
            if i == j:
                ax.plot(freqs, np.abs(spectra[i, i, :]), color="k")
            else:
                ax.fill_between(freqs, ff_dtf[i, j, :], color="C0")
                ax.set_ylim(0, top)
            ax.tick_params(labelsize=5)
            if i == 0:
                ax.set_title(names[j], fontsize=7)
            if j == 0:
                ax.set_ylabel(names[i], fontsize=7)
    fig.suptitle(top_title, fontsize=9)
    return fig


def compute_and_plot_mvar(ncdf_path, channel_subset=None, max_model_order=20, optimal_model_order=None,
                          crit_type="AIC", freq_min=1.0, freq_max=40.0, freq_step=0.5, low_cutoff_hz=None,
                          high_cutoff_hz=None, plot=True, plot_loaded_signal=False, loaded_signal_max_channels=19,
                          loaded_signal_spacing=8.0, loaded_signal_figsize=(16.0, 9.0), loader=None):
    """Load one EEG NetCDF file, compute ffDTF and multivariate spectra, optionally plot (mtmvar.py:1006-1128).

    Returns (ff_dtf, spectra, chan_names, crit, model_order_range, p_opt) like the reference.  The
    reference imports its loader from a module that does not define it; here it is wired
    to `eeg_io.load_eeg_signals` (same semantics as `src/mne_bridge.py:113-223`), or to `loader=` if given.
    One fit feeds both products.
    """
    if loader is None:
        from .eeg_io import load_eeg_signals as loader
    signals, chan_names, fs, time_s, event_duration_s = loader(
        ncdf_path, channel_subset=channel_subset, low_cutoff_hz=low_cutoff_hz, high_cutoff_hz=high_cutoff_hz)
    stem = ncdf_path.stem if hasattr(ncdf_path, "stem") else ncdf_path
    if plot_loaded_signal:
        import matplotlib.pyplot as plt
        k = min(loaded_signal_max_channels, signals.shape[0])
        plt.figure(figsize=loaded_signal_figsize)
        for c in range(k):
            plt.plot(time_s, signals[c] - c * loaded_signal_spacing, lw=0.6)
        plt.yticks([-c * loaded_signal_spacing for c in range(k)], chan_names[:k])
        plt.axvline(event_duration_s, color="r", lw=0.8)
        plt.title(f"Loaded EEG signal — {stem}")
        plt.show()
    freqs = np.arange(freq_min, freq_max + freq_step, freq_step)
    print(f"\n  Channels : {chan_names}")
    print(f"  Signals  : {signals.shape}  fs={fs} Hz")
    if optimal_model_order is None:
        crit, model_order_range, p_opt = mvar_criterion(signals, max_model_order, crit_type, plot=False)
        print(f"  {crit_type} optimal model order: p = {p_opt}")
    else:
        p_opt = optimal_model_order
        print(f"  Using fixed model order: p = {p_opt}")
        crit = np.array([])
        model_order_range = np.array([])
    print("  Computing ffDTF ...")
    print("  Computing multivariate spectra ...")
    res = mvar_analysis(signals, freqs, fs, int(p_opt), want=("ffdtf", "spectra"))
    ff_dtf, spectra = res["ffdtf"], res["spectra"]
    if plot:
        import matplotlib.pyplot as plt
        mvar_plot(spectra, ff_dtf, freqs, chan_names, top_title=f"MVAR Spectra and ff_DTF — {stem}")
        plt.suptitle(f"{stem}  (fs={fs:.0f} Hz, {signals.shape[0]} ch, {signals.shape[1]} samp)", fontsize=8, y=1.01)
        plt.tight_layout()
        plt.show()
    return ff_dtf, spectra, chan_names, crit, model_order_range, p_opt


# ----------------------------------------------------------------------------- FAD decomposition (mtmvar.py:607-845)
_FAD_POLE_KEYS = ("poles", "C", "alpha", "freq_hz", "omega_rad_s", "beta", "bandwidth_hz", "phi", "B")


def block_granger_causality(signals, freqs, fs, split, max_model_order=20, optimal_model_order=None, crit_type='AIC'):
    """Block (multivariate) Granger causality between the channels < split (block A) and the channels >= split (block B)
    of one window signals (channels, samples) -- Geweke (1982); beyond the reference, in its signature style.  The order is
    `optimal_model_order`, or with None the one `mvar_criterion(signals, max_model_order, crit_type)` selects first.
    Returns (spectral (2, F), time (4,)): spectral[0] = f_{A->B}(f), spectral[1] = f_{B->A}(f) on the spectrum
    S = H V H^H (CONJUGATE transpose: not the plain transpose that `multivariate_spectra` reproduces); time =
    (F_{A->B}, F_{B->A}, F_{A.B}, F_{A,B}) from the residual covariances of the full fit and of the same-order Yule-Walker
    fits of each block alone (the classical Geweke estimator, not the state-space / spectral-factorisation one)."""
    from .engine import check_block_split
    signals = _one_window(signals, "block_granger_causality")
    split = check_block_split(split, signals.shape[0], "block_granger_causality")
    p = _order(signals, max_model_order, optimal_model_order, crit_type, False, None, "dtf")
    eng = default_engine()
    x = _as_trials(signals, eng)
    zero = torch.zeros(1, dtype=torch.int64, device=eng.device)
    spectral, time = eng.sliding_block_granger(x, zero, zero, signals.shape[1], p, np.asarray(freqs, dtype=np.float64), fs,
                                               split=split)
    return spectral[0].cpu().numpy(), time[0].cpu().numpy()


def _fad_orders(model_order, max_model_order, crit_type, n):
    """(order code, pmax, crit code) for hmv_fad_f64, with the reference's ValueError for an unknown criterion."""
    if model_order is None:
        if crit_type not in Engine.FAD_CRIT:
            raise ValueError("Invalid criterion type. Choose from 'AIC', 'HQ', 'SC'.")
        order, pmax, crit = 0, int(max_model_order), Engine.FAD_CRIT[crit_type]
    else:
        order = pmax = int(model_order)
        crit = 0
    if not 1 <= pmax <= 32:
        raise ValueError(f"FAD supports model orders 1..32, got {pmax}")
    if n <= pmax:
        raise ValueError(f"need more samples ({n}) than the model order ({pmax})")
    return order, pmax, crit


def _fad_host(d: dict, model_order, pair_conjugates: bool):
    """Device dict of Engine.fad -> the reference's dict layout with a leading series axis (NumPy, padded rows)."""
    h = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    S, P = h["freq_hz"].shape
    orders = h["order"].astype(np.int64) if "order" in h else np.full(S, P, dtype=np.int64)
    out = {
        "model_order": orders,
        "poles": h["poles"], "C": h["C"], "alpha": h["alpha"], "freq_hz": h["freq_hz"],
        "omega_rad_s": h["alpha"].imag.copy(), "beta": h["beta"], "bandwidth_hz": h["bandwidth_hz"],
        "phi": h["phi"], "B": h["B"],
        "noise_variance": h.get("noise_variance"),
        "osc_mask": h["osc_mask"],
        "ar_coeffs": h.get("ar"),
    }
    idx = h["paired_index"].astype(np.int64)
    have = idx >= 0
    safe = np.where(have, idx, 0)
    paired = {"pole_index": np.where(have, idx, -1)}
    for k in _FAD_POLE_KEYS:
        v = np.take_along_axis(out[k], safe, axis=1)
        paired[k] = np.where(have, v, np.nan)
    paired["n_components"] = h["n_paired"].astype(np.int64)
    out["paired_components"] = paired
    out["info"] = h["info"]
    if h.get("crit") is not None:
        out["crit"] = h["crit"]
    return out


def _fad_run(signals, fs, model_order, max_model_order, crit_type, pair_conjugates, imag_tol, eng: Engine | None):
    x = np.ascontiguousarray(np.asarray(signals, dtype=np.float64))
    S, n = x.shape
    order, pmax, crit = _fad_orders(model_order, max_model_order, crit_type, n)
    eng = eng or default_engine()
    xd = eng.to_device(x[:, None, :])                                  # S recordings of one channel
    rec = torch.arange(S, dtype=torch.int64, device=eng.device)
    start = torch.zeros(S, dtype=torch.int64, device=eng.device)
    d = eng.fad(xd, rec, start, n, pmax, order, crit, fs, imag_tol, pair_conjugates)
    return _fad_host(d, model_order, pair_conjugates), order


def fad_decomposition_batch(signals, fs, model_order=None, max_model_order=20, crit_type='AIC', pair_conjugates=True,
                            imag_tol=1e-8, engine: Engine | None = None):
    """`fad_decomposition` of every row of signals (S, N) in one pass on the GPU.

    Same keys as `fad_decomposition` with a leading (S,) axis: per-pole arrays (S, pmax), NaN-padded past each
    series' order (`osc_mask` padded with False), `model_order` (S,) int64, `noise_variance` (S,), `ar_coeffs`
    (S, pmax); `paired_components` arrays (S, pmax) padded with NaN (`pole_index` with -1) plus `n_components` (S,);
    `info` (S,) (bit 0: fit breakdown, bit 1: root iteration did not converge, bit 2: ambiguous pole grouping) and,
    in automatic mode, `crit` (S, max_model_order).  pmax is max_model_order in automatic mode, else model_order.
    Nothing is printed and nothing is raised for individual series: failed rows are NaN and flagged in `info`.
    Row s is bit-for-bit what `fad_decomposition(signals[s], ...)` returns.
    """
    x = np.asarray(signals, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("signals must have shape (n_series, n_samples)")
    out, _ = _fad_run(x, fs, model_order, max_model_order, crit_type, pair_conjugates, imag_tol, engine)
    return out


def fad_decomposition(signal, fs, model_order=None, max_model_order=20, crit_type='AIC', plot=False,
                      pair_conjugates=True, imag_tol=1e-8):
    """FAD (frequency-amplitude-damping) decomposition of a univariate AR model (mtmvar.py:607-757).

    Same signature, defaults, dict keys, shapes, dtypes, printed line and errors as the reference: the AR fit
    (order by AIC / HQ / SC when model_order is None), the poles z_j and residues C_j of H(z) = 1 / A(z^-1) as
    scipy.signal.residuez returns them, alpha = log(z) fs, beta = -Re alpha, omega = Im alpha, freq_hz = omega / 2 pi,
    bandwidth_hz = beta / 2 pi, phi = arg C, B = 2 |C|, osc_mask and `paired_components`.  The fit (Levinson-Durbin)
    and the root finding (Aberth-Ehrlich) run on the GPU; results agree with the reference to rounding.
    Raises numpy.linalg.LinAlgError('Singular matrix') when the fit breaks down (all-zero input), RuntimeError when
    the root iteration does not converge, and warns (RuntimeWarning) when poles form a chain within 1e-3 that is wider
    than 1e-3 (residuez's grouping then depends on the root order; here connected components are grouped).
    """
    x = np.atleast_2d(np.asarray(signal, dtype=float))
    if x.shape[0] != 1:
        raise ValueError("fad_decomposition expects a univariate signal, shape (N,) or (1, N).")
    b, order = _fad_run(x, fs, model_order, max_model_order, crit_type, pair_conjugates, imag_tol, None)
    info = int(b["info"][0])
    if info & 1:
        raise SingularMatrixError("Singular matrix")
    if info & 2:
        raise RuntimeError("fad_decomposition: the root iteration did not converge")
    if info & 4:
        import warnings
        warnings.warn("fad_decomposition: poles within 1e-3 of each other form a chain wider than 1e-3; grouped by "
                      "connected components", RuntimeWarning, stacklevel=2)
    p = int(b["model_order"][0])
    if model_order is None:
        if plot:
            crit = b["crit"][0]
            _criterion_figure(np.arange(1, len(crit) + 1), crit, int(np.argmin(crit)), crit_type)
        print(f'FAD: optimal AR model order ({crit_type}) = {p}')
        model_order = np.int64(p)                  # what the reference's arg-min over an int array gives
    k = int(b["paired_components"]["n_components"][0])
    paired = {key: b["paired_components"][key][0, :k].copy() for key in ("pole_index",) + _FAD_POLE_KEYS}
    fad_params = {
        'model_order': model_order,
        **{key: b[key][0, :p].copy() for key in _FAD_POLE_KEYS},
        'noise_variance': float(b["noise_variance"][0]),
        'osc_mask': b["osc_mask"][0, :p].copy(),
        'ar_coeffs': b["ar_coeffs"][0, :p].copy(),
        'paired_components': paired,
    }
    if plot:
        _fad_figure(x.ravel(), fs, fad_params)
    return fad_params


def fad_components_table(fad_params, output='dataframe', decimals=None):
    """One row per entry of fad_params['paired_components'] (mtmvar.py:759-842), columns
    component, freq_hz, omega_rad_s, beta_s_1, bandwidth_hz, B, phi_rad, pole_real, pole_imag, residue_real,
    residue_imag; `output` 'ndarray' (float array, the columns in this order) or 'dataframe' (pandas, integer
    `component`); `decimals` rounds every value."""
    pc = fad_params.get('paired_components', None)
    if pc is None:
        raise ValueError("fad_params does not contain 'paired_components'.")
    rows = len(pc['freq_hz'])
    cols = [np.arange(1, rows + 1, dtype=int), pc['freq_hz'], pc['omega_rad_s'], pc['beta'], pc['bandwidth_hz'],
            pc['B'], pc['phi'], np.real(pc['poles']), np.imag(pc['poles']), np.real(pc['C']), np.imag(pc['C'])]
    table = np.column_stack(cols)
    if decimals is not None:
        table = np.round(table, decimals=decimals)
    if output == 'ndarray':
        return table
    if output != 'dataframe':
        raise ValueError("output must be 'dataframe' or 'ndarray'.")
    try:
        import pandas as pd
    except ImportError as exc:
        raise ImportError("pandas is required for output='dataframe'. Use output='ndarray' instead.") from exc
    df = pd.DataFrame(table, columns=FAD_TABLE_COLUMNS)
    df['component'] = df['component'].astype(int)
    return df


FAD_TABLE_COLUMNS = ['component', 'freq_hz', 'omega_rad_s', 'beta_s_1', 'bandwidth_hz', 'B', 'phi_rad', 'pole_real',
                     'pole_imag', 'residue_real', 'residue_imag']


def _fad_figure(signal, fs, fad):
    """The figure of fad_decomposition(..., plot=True): poles against the unit circle (left), the AR spectrum
    sigma^2 / |A(f)|^2 with every oscillator's frequency, half-power bandwidth and amplitude marked (right)."""
    import matplotlib.pyplot as plt
    z = fad['poles']
    pc = fad['paired_components']
    up = np.imag(pc['poles']) > 1e-8                 # one marker per conjugate pair, whatever pair_conjugates was
    comp = {key: np.asarray(pc[key])[up] for key in ('pole_index', 'freq_hz', 'B', 'bandwidth_hz')}
    colors = plt.cm.viridis(np.linspace(0.15, 0.9, max(len(comp['freq_hz']), 1)))
    f = np.linspace(0.0, fs / 2.0, 1025)
    a = np.asarray(fad['ar_coeffs'])
    A = 1.0 - np.exp(-2j * np.pi * np.outer(f / fs, np.arange(1, len(a) + 1))) @ a
    spec = fad['noise_variance'] / np.abs(A) ** 2
    fig, (ax0, ax1) = plt.subplots(1, 2, figsize=(13, 5))
    fig.suptitle(f"FAD decomposition  (AR order p = {fad['model_order']})", fontsize=13)
    t = np.linspace(0.0, 2.0 * np.pi, 300)
    ax0.plot(np.cos(t), np.sin(t), "k-", lw=0.9, alpha=0.4)
    ax0.axhline(0, color="k", lw=0.5, alpha=0.4)
    ax0.axvline(0, color="k", lw=0.5, alpha=0.4)
    real = ~np.asarray(fad['osc_mask'])
    ax0.scatter(z[real].real, z[real].imag, color="gray", s=40, marker="s", zorder=4)
    for c, j, fj in zip(colors, comp['pole_index'], comp['freq_hz']):
        ax0.scatter(z[j].real, z[j].imag, color=c, s=70, zorder=5, label=f"{fj:.2f} Hz")
        ax0.scatter(z[j].real, -z[j].imag, color=c, s=70, zorder=5, marker="x")
    ax0.set(xlim=(-1.25, 1.25), ylim=(-1.25, 1.25), xlabel="Re(z)", ylabel="Im(z)", title="Poles in the complex plane")
    ax0.set_aspect("equal")
    if len(comp['freq_hz']):
        ax0.legend(fontsize=8, loc="upper left", title="freq [Hz]")
    ax0.grid(True, alpha=0.3)
    ax1.plot(f, spec, "k-", lw=1.5, label="AR spectrum")
    for c, fj, bj, bw in zip(colors, comp['freq_hz'], comp['B'], comp['bandwidth_hz']):
        peak = spec[np.argmin(np.abs(f - fj))]
        ax1.plot([fj, fj], [0, peak], color="r", lw=1.2, alpha=0.9)
        ax1.plot([max(0.0, fj - bw), min(fs / 2.0, fj + bw)], [peak / 2, peak / 2], color="m", lw=1.8, alpha=0.9)
        ax1.scatter([fj], [peak], color=c, s=28, zorder=6)
        ax1.annotate(f"{fj:.1f} Hz\nBW={bw:.2f} Hz\nB={bj:.3g}", xy=(fj, peak), xytext=(6, 8),
                     textcoords="offset points", fontsize=7, color=c)
    ax1.set(xlabel="Frequency [Hz]", ylabel="Power", title="AR spectrum and FAD components", xlim=(0, fs / 2.0))
    ax1.legend(fontsize=8)
    ax1.grid(True, alpha=0.3)
    fig.tight_layout()
    plt.show()
    return fig
