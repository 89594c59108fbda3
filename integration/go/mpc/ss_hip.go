//go:build hip

// Drop-in bodies of the two encoder steps of mpc/ss.go (row f-4 of SURVEY.md §8): ss.go:114-134 (EncodeRVecNew of the party's share, inside SSToCMat) and
// ss.go:239-279 (KeySwitch, Plaintext, DecodeRVec and the subtraction, inside CMatToSS).  The surrounding network steps - RevealSymMat, EncryptPlaintextMatrix +
// AggregateCMat, AggregateRefreshShareVec - stay as they are.  NOT COMPILED in the sfgwas-hip repository.  PARITY UNPINNED against the fork's encoder.
package mpc

import (
	"github.com/hhcho/sfgwas/crypto"
	"github.com/hhcho/sfgwas/hip"
	"github.com/ldsec/lattigo/v2/ckks"
	"github.com/ldsec/lattigo/v2/ring"
	mpc_core "github.com/hhcho/mpc-core"
)

// encodeShareHip replaces ss.go:114-134: the rows of `share` cut into plaintexts of at most `slots` elements, encoded at MaxLevel with the default scale.
func (mpcObj *MPC) encodeShareHip(cryptoParams *crypto.CryptoParams, share mpc_core.RMat) crypto.PlainMatrix {
	h := hip.Default
	t := share.Type()
	limbs := limbsOf(t)
	mod := modulusLimbs(t, limbs)
	slots := cryptoParams.GetSlots()
	level := cryptoParams.Params.MaxLevel()
	scale := cryptoParams.Params.Scale()
	nElemCol := len(share[0])
	numCtxCol := 1 + ((nElemCol - 1) / slots)
	pm := make(crypto.PlainMatrix, len(share))
	for i := range share {
		pm[i] = make(crypto.PlainVector, numCtxCol)
		for j := 0; j < numCtxCol; j++ {
			start, end := j*slots, (j+1)*slots
			if end > nElemCol {
				end = nElemCol
			}
			flat := toLimbs(mpc_core.RMat{share[i][start:end]}, limbs)
			words := h.EncodeRVec(limbs, mod, flat, end-start, 1, level, scale, mpcObj.GetFracBits())
			pt := ckks.NewPlaintext(cryptoParams.Params, level, scale)
			for m := 0; m <= level; m++ {
				copy(pt.Value()[0].Coeffs[m], words[m*h.N:(m+1)*h.N])
			}
			pm[i][j] = pt
		}
	}
	return pm
}

// decodeSharesHip replaces ss.go:239-279: cm at levelStart, agg the aggregated decryption shares, ctMask the NTT-domain masks of this party.
func (mpcObj *MPC) decodeSharesHip(cryptoParams *crypto.CryptoParams, rtype mpc_core.RElem, cm crypto.CipherMatrix, agg [][]*ring.Poly,
	ctMask crypto.CipherMatrix, levelStart, numCtxRow, nElemRow int) mpc_core.RMat {
	h := hip.Default
	limbs := limbsOf(rtype)
	mod := modulusLimbs(rtype, limbs)
	slots := cryptoParams.GetSlots()
	isHub := mpcObj.GetPid() == mpcObj.GetHubPid()
	rm := mpc_core.InitRMat(rtype.Zero(), numCtxRow, nElemRow)
	rowWords := (levelStart + 1) * h.N
	for i := range cm {
		nct := len(cm[i])
		maskFlat := make([]uint64, nct*rowWords)
		aggFlat := make([]uint64, nct*rowWords)
		for j := range cm[i] {
			for m := 0; m <= levelStart; m++ {
				copy(maskFlat[j*rowWords+m*h.N:], ctMask[i][j].Value()[0].Coeffs[m])
				copy(aggFlat[j*rowWords+m*h.N:], agg[i][j].Coeffs[m])
			}
		}
		var ctFlat []uint64
		if isHub {
			ctFlat = h.FlattenVec(cm[i], nct, levelStart)
		}
		out := h.CKKSToSSFinish(limbs, mod, ctFlat, nct, levelStart, cm[i][0].Scale(), mpcObj.GetFracBits(), aggFlat, maskFlat, isHub, slots)
		row := fromLimbs(rtype, out, 1, nct*slots, limbs)[0]
		for k := 0; k < nElemRow && k < nct*slots; k++ {
			rm[i][k] = row[k]
		}
	}
	return rm
}
