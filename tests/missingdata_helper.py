"""The missing-data treatment of the ELB months (doELBsampling = false:
mcmcVARshadowrateBlockHybrid.m:481-499, mcmcVARhybridGibbs.m:499-518, mcmcVARshadowrate.m:442-459)
restated on the oracle's sweeps: the sweep's one unconstrained draw of the censored cells
(out["missingrate"], the precision sampler at crn["zPS"], one column) becomes the data of the next
sweep whatever the accept test of the PS branch says, and shadowrate is NaN (:492)."""
import numpy as np


def missing_sweep(mod, st, setup, crn, cta_form="mirror", hybrid=False):
    """One sweep under the treatment.  mod: oracle.ccmm_oracle_bh (block hybrid; the shadow-rate
    model is the block hybrid with an empty actual-rate block) or oracle.ccmm_oracle_hybrid."""
    assert crn["zPS"].shape[1] == 1, "one draw per sweep"
    if hybrid:
        out = mod.hybrid_sweep(st, setup, crn, elb_impl="stable", use_ps=True, cta_form=cta_form)
    else:
        out = mod.bh_sweep(st, setup, crn, elb_impl="stable", use_ps=True, cta_form=cta_form)
    X, Y = mod.rebuild_XY(setup, out["missingrate"])
    out.update(X=X, Y=Y, shadowrate=np.full_like(out["missingrate"], np.nan), path=out["missingrate"])
    return out


def draw_crn(mod, rng, setup, hybrid=False):
    return mod.hybrid_draw_crn(rng, setup, 1) if hybrid else mod.bh_draw_crn(rng, setup, 1)


def crn_record(mod, setup, crn, NP=1, hybrid=False, zalt=None):
    """Device CRN record of one sweep: the linear blocks, uELB (present, unread under the treatment),
    zPS (nmiss x NP) padded to Ns elbT NP, then (alternate draw) zALT padded to Ns elbT."""
    sizes = mod.hybrid_crn_sizes(setup) if hybrid else mod.bh_crn_sizes(setup)
    parts = [crn[k].ravel(order="F") for k, _ in sizes]
    per = len(setup.ndxS) * setup.elbT
    for z, n in ((crn.get("zPS"), per * NP), (zalt, per)):
        if z is not None:
            z = np.asarray(z, float).ravel(order="F")
            parts.append(np.concatenate([z, np.zeros(n - z.size)]))
    return np.concatenate(parts)
