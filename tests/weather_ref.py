"""numpy reference of the weather / parameter variance split (ps_nested_*, predictive.WeatherShare): the statements
of include/parasitoid_hip.h executed one operation at a time in IEEE double -- numpy rounds every operation on its
own -- so that every plane of the device handle can be compared bit for bit; and the closed forms they estimate."""
import numpy as np


class NestedReplay():
    '''the planes of one slot, or of a stack of slots: any array shape'''

    def __init__(self, shape):
        self.imean, self.iM2 = np.zeros(shape), np.zeros(shape)
        self.omean, self.oM2, self.wS = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        self.k = self.G = self.members = 0
        self.W = self.wk = 0.0

    def add(self, v):
        v = np.asarray(v, dtype=np.float64)
        kn = float(self.k + 1)
        d = v - self.imean
        ch = d != 0.0
        m = np.where(ch, self.imean + d / kn, self.imean)
        self.iM2 = np.where(ch, self.iM2 + d * (v - m), self.iM2)
        self.imean = m
        self.k += 1
        self.members += 1

    def close(self, w):
        assert self.k >= 2
        w = float(w)
        s2 = self.iM2 / float(self.k - 1)
        self.wS = self.wS + w * s2
        Wn = self.W + w
        d = self.imean - self.omean
        ch = d != 0.0
        g = np.where(ch, self.omean + (d * w) / Wn, self.omean)
        self.oM2 = np.where(ch, self.oM2 + (w * d) * (self.imean - g), self.oM2)
        self.omean = g
        self.imean, self.iM2 = np.zeros_like(self.imean), np.zeros_like(self.iM2)
        self.wk += w / float(self.k)
        self.W = Wn
        self.G += 1
        self.k = 0

    def merge(self, other):
        assert self.k == 0 and other.k == 0
        if other.G > 0:
            if self.G == 0:
                self.omean, self.oM2, self.wS = other.omean.copy(), other.oM2.copy(), other.wS.copy()
            else:
                W = self.W + other.W
                fb = other.W / W
                fab = (self.W * other.W) / W
                d = other.omean - self.omean
                self.omean = self.omean + d * fb
                self.oM2 = (self.oM2 + other.oM2) + (d * d) * fab
                self.wS = self.wS + other.wS
        self.G += other.G
        self.W += other.W
        self.wk += other.wk
        self.members += other.members

    def finalize(self):
        '''-> dict(vw, vm, vp, share)'''
        assert self.k == 0 and self.G >= 2
        kinv = self.wk / self.W
        vw = self.wS / self.W
        vm = self.oM2 / self.W
        vp = vm - vw * kinv
        vp = np.where(vp > 0.0, vp, 0.0)
        tot = vp + vw
        share = np.where(tot > 0.0, vw / np.where(tot > 0.0, tot, 1.0), 0.0)
        return dict(vw=vw, vm=vm, vp=vp, share=share)

    def planes(self):
        return dict(imean=self.imean, iM2=self.iM2, omean=self.omean, oM2=self.oM2, wS=self.wS)


def closed_form(groups, weights):
    '''groups: per group an array [k_g, ...] of its draws; -> dict(vw, vm, vp, share, mean) in plain float64
    formulas: vw = sum w_g s2_g / W with the sample variance s2_g, vm = sum w_g (m_g - m)^2 / W,
    vp = max(vm - vw (sum w_g / k_g) / W, 0)'''
    w = np.asarray(weights, dtype=np.float64)
    W = w.sum()
    means = np.array([np.mean(g, axis=0) for g in groups])
    s2 = np.array([np.var(g, axis=0, ddof=1) for g in groups])
    shape = (-1,) + (1,) * (means.ndim - 1)
    ww = w.reshape(shape)
    mean = (ww * means).sum(0) / W
    vw = (ww * s2).sum(0) / W
    vm = (ww * (means - mean) ** 2).sum(0) / W
    kinv = sum(wg / len(g) for wg, g in zip(w, groups)) / W
    vp = np.maximum(vm - vw * kinv, 0.0)
    tot = vp + vw
    share = np.where(tot > 0, vw / np.where(tot > 0, tot, 1.0), 0.0)
    return dict(vw=vw, vm=vm, vp=vp, share=share, mean=mean)
