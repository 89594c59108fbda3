//go:build hip

// Package hip is the cgo binding of libsfgwas_hip.so (include/sfgwas_hip.h) for hhcho/sfgwas.
//
// Where it goes: copy this directory to github.com/hhcho/sfgwas/hip and the sibling files to gwas/, crypto/ and mpc/
// (each carries the build tag `hip`; the files they replace get `//go:build !hip`, see INTEGRATION.md §0).
//
// NOT COMPILED IN THE sfgwas-hip REPOSITORY: its image has no Go toolchain and the lattigo fork / mpc-core modules are not
// vendored in the reference tree.  The lattigo API used here is the one the reference itself uses (ckks.Ciphertext.Value()[k].Coeffs[l],
// ckks.NewCiphertext, ckks.RotationKeySet.Keys, ckks.SwitchingKey.Value, ring.NewRing / PsiMont / MredParams / InvMForm); a maintainer
// should expect to fix small spelling differences against the fork on the first build.
//
// This package imports lattigo only (never sfgwas/crypto, gwas or mpc), so all three can import it without a cycle.
package hip

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/sfgwas-hip/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/sfgwas-hip/sfgwas_amd/lib -lsfgwas_hip -Wl,-rpath,${SRCDIR}/../third_party/sfgwas-hip/sfgwas_amd/lib
#include <stdlib.h>
#include "sfgwas_hip.h"
*/
import "C"

import (
	"crypto/rand"
	"fmt"
	"sync"
	"unsafe"

	"github.com/ldsec/lattigo/v2/ckks"
	"github.com/ldsec/lattigo/v2/ring"
)

// Ctx is one caller's handle on the library: tables and keys are shared between forks, queues and scratch are per handle.
// The reference runs MatMult4Stream from several goroutines at once (gwas/assoc.go:360-408): each takes its own Fork().
type Ctx struct {
	p      *C.sfg_ctx
	mg     *C.sfg_mgpu // non-nil when Init was given several devices: the products and the association scan run on all of them (include/sfgwas_hip.h, "SURVEY 8e")
	Params *ckks.Parameters
	N      int // ring degree
	NQ, NP int // moduli of Q and of P
}

// Default is the context the drop-in function bodies use; Init sets it (gwas/gwas.go:212, after CollectiveInit).
var Default *Ctx

// check converts a non-zero return code into a panic: the reference panics / log.Fatals on this path
// (gwas/matmult.go:361, gwas/filestream.go:60,334, crypto/basics.go:817), it never returns errors.
func (h *Ctx) check(rc C.int, what string) {
	if rc != 0 {
		panic(fmt.Sprintf("sfgwas-hip: %s: %s", what, C.GoString(C.sfg_last_error(h.p))))
	}
}

// Init creates the device context(s) from the CKKS parameters and uploads every switching key the party holds.
//   rotKs: cryptoParams.RotKs (crypto/crypto.go:50, filled at :208), rlk: cryptoParams.Rlk (:49).
//   devices: the HIP devices of this party's node.  One device: a plain context.  Several: the multi-GPU engine (sfg_mgpu_create: one context per device,
//   RCCL inside the library) - the genotype matrix registered by MatMult4StreamPreprocess is sharded by SNP block over them, MatMult4StreamCompute and the
//   association scan run on all of them, and everything else (evaluator ops, per-call MatMult4Stream forks) runs on devices[0]'s context.
func Init(params *ckks.Parameters, rotKs *ckks.RotationKeySet, rlk *ckks.RelinearizationKey, devices []int) *Ctx {
	if len(devices) == 0 {
		devices = []int{0}
	}
	qi, pi := params.Qi(), params.Pi()
	moduli := append(append([]uint64{}, qi...), pi...)
	ringQP, err := ring.NewRing(params.N(), moduli)
	if err != nil {
		panic(err)
	}
	// lattigo's own primitive 2N-th roots, out of Montgomery form: the NTT output order then is lattigo's, whichever root its
	// parameter generation picked (include/sfgwas_hip.h: sfg_ctx_create, `psi`)
	psi := make([]uint64, len(moduli))
	for i := range moduli {
		psi[i] = ring.InvMForm(ringQP.PsiMont[i], moduli[i], ringQP.MredParams[i])
	}
	h := &Ctx{Params: params, N: params.N(), NQ: len(qi), NP: len(pi)}
	if len(devices) == 1 {
		var c *C.sfg_ctx
		if C.sfg_ctx_create(&c, C.int(devices[0]), C.int(params.LogN()), C.int(len(qi)), C.int(len(pi)),
			(*C.uint64_t)(unsafe.Pointer(&moduli[0])), (*C.uint64_t)(unsafe.Pointer(&psi[0])), C.double(params.Scale())) != 0 {
			panic("sfgwas-hip: sfg_ctx_create: " + C.GoString(C.sfg_last_error(nil)))
		}
		h.p = c
	} else {
		devs := make([]C.int, len(devices))
		for i, d := range devices {
			devs[i] = C.int(d)
		}
		var m *C.sfg_mgpu
		if C.sfg_mgpu_create(&m, &devs[0], C.int(len(devs)), C.int(params.LogN()), C.int(len(qi)), C.int(len(pi)),
			(*C.uint64_t)(unsafe.Pointer(&moduli[0])), (*C.uint64_t)(unsafe.Pointer(&psi[0])), C.double(params.Scale())) != 0 {
			panic("sfgwas-hip: sfg_mgpu_create: " + C.GoString(C.sfg_mgpu_last_error(nil)))
		}
		h.mg = m
		h.p = C.sfg_mgpu_ctx(m, 0)
	}
	if rotKs != nil {
		for galEl, swk := range rotKs.Keys {
			flat := FlattenSwitchingKey(swk, h.NQ+h.NP, h.N)
			if h.mg != nil {
				h.mcheck(C.sfg_mgpu_load_rotkey(h.mg, C.uint64_t(galEl), (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "mgpu_load_rotkey")
			} else {
				h.check(C.sfg_ctx_load_rotkey(h.p, C.uint64_t(galEl), (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "load_rotkey")
			}
		}
	}
	if rlk != nil && len(rlk.Keys) > 0 {
		flat := FlattenSwitchingKey(rlk.Keys[0], h.NQ+h.NP, h.N)
		if h.mg != nil {
			h.mcheck(C.sfg_mgpu_load_relinkey(h.mg, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "mgpu_load_relinkey")
		} else {
			h.check(C.sfg_ctx_load_relinkey(h.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "load_relinkey")
		}
	}
	Default = h
	return h
}

// LoadPublicKey gives the device cryptoParams.Pk (crypto/crypto.go:45: [2] polynomials over QP, NTT + Montgomery form) and seeds its sampler with 32 bytes of
// crypto/rand - the source lattigo's own encryptor draws from (crypto.go:355 NewEncryptorFromPk).  Call it once per process right after Init (gwas/gwas.go:212);
// Init keeps its four arguments.  A process that restarts MUST come through here again: the encryption index restarts at 0, and an index may be used only once
// per key, so the key has to be fresh (INTEGRATION.md, "Encrypting on the device").  With several devices the products are finished on devices[0]'s context.
func (h *Ctx) LoadPublicKey(pk *ckks.PublicKey) {
	nmod := h.NQ + h.NP
	flat := make([]uint64, 2*nmod*h.N)
	for k := 0; k < 2; k++ {
		for m := 0; m < nmod; m++ {
			copy(flat[(k*nmod+m)*h.N:(k*nmod+m+1)*h.N], pk.Value[k].Coeffs[m])
		}
	}
	h.check(C.sfg_ctx_load_public_key(h.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "load_public_key")
	var key [32]byte
	if _, err := rand.Read(key[:]); err != nil {
		panic(err)
	}
	h.check(C.sfg_ctx_seed_encryptor(h.p, (*C.uint8_t)(unsafe.Pointer(&key[0]))), "seed_encryptor")
	for i := range key {
		key[i] = 0
	}
}

// CanEncrypt: a public key is loaded (and with it, by LoadPublicKey, a sampler key): products are finished on the device.
func (h *Ctx) CanEncrypt() bool { return C.sfg_ctx_has_public_key(h.p) != 0 }

// AddFreshZero: crypto.CZeroMat + eval.Add (basics.go:367-384; matmult.go:1174,1225,1443,1494) on the device - every one of the nct ciphertexts of flat
// ([nct][2][level+1][N]) gets a fresh encryption of zero added; the words never visit lattigo's Add.
func (h *Ctx) AddFreshZero(flat []uint64, nct, level int) []uint64 {
	d := h.Upload(flat)
	defer d.Free()
	h.check(C.sfg_ct_add_fresh_zero_dev(h.p, d.U64(), C.int(nct), C.int(level)), "add_fresh_zero")
	return d.Download()
}

// EncryptFloatVector: crypto.EncryptFloatVector (crypto.go:340-362) - f packed into ceil(len/slots) ciphertexts at `level` (the reference: MaxLevel), default scale.
func (h *Ctx) EncryptFloatVector(f []float64, level int) []*ckks.Ciphertext {
	slots := h.N / 2
	nvec := (len(f) + slots - 1) / slots
	padded := make([]float64, nvec*slots)
	copy(padded, f)
	d := h.Alloc(nvec * h.CtWords(level) * 8)
	defer d.Free()
	h.check(C.sfg_encrypt_vectors_dev(h.p, (*C.double)(unsafe.Pointer(&padded[0])), C.int(nvec), C.int(level), d.U64()), "encrypt_vectors")
	return h.VecFromFlat(d.Download(), nvec, level, h.Params.Scale())
}

// LoadSecretKey gives the device cryptoParams.Sk (crypto/crypto.go:44, NTT + Montgomery form): this party's shard for the collective calls, the whole key for
// DecryptFloatVector.
func (h *Ctx) LoadSecretKey(sk *ckks.SecretKey) {
	flat := make([]uint64, h.NQ*h.N)
	for m := 0; m < h.NQ; m++ {
		copy(flat[m*h.N:(m+1)*h.N], sk.Value.Coeffs[m])
	}
	h.check(C.sfg_ctx_load_secret_key(h.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "load_secret_key")
}

// DecodeFloatVector: crypto.DecodeFloatVector (crypto.go:525-536) - the real parts of every slot of nvec NTT-domain plaintexts ([nvec][level+1][N] words).
func (h *Ctx) DecodeFloatVector(flat []uint64, nvec, level int, scale float64) []float64 {
	d := h.Upload(flat)
	defer d.Free()
	out := make([]float64, nvec*h.N/2)
	h.check(C.sfg_decode_vectors(h.p, d.U64(), C.size_t((level+1)*h.N), C.int(nvec), C.int(level), C.double(scale), (*C.double)(unsafe.Pointer(&out[0])), nil), "decode_vectors")
	return out
}

// DecryptFloatVector: crypto.DecryptFloatVector (crypto.go:489-510) under the loaded key - nct ciphertexts ([nct][2][level+1][N] words) to nct * slots reals.
func (h *Ctx) DecryptFloatVector(flat []uint64, nct, level int, scale float64) []float64 {
	d := h.Upload(flat)
	defer d.Free()
	out := make([]float64, nct*h.N/2)
	h.check(C.sfg_decrypt_vectors(h.p, d.U64(), C.int(nct), C.int(level), C.double(scale), (*C.double)(unsafe.Pointer(&out[0])), nil), "decrypt_vectors")
	return out
}

// PCKSGenShare: the local half of mpc.CollectiveDecrypt* before the aggregation (mhe.go:107-220: PCKSProtocol.GenShare with the zero public key); e0 holds the
// caller's Gaussian draws, [nct][N].  Returns polynomial 0 of every share, [nct][level+1][N]; polynomial 1 is discarded by the reference and not computed.
func (h *Ctx) PCKSGenShare(flat []uint64, nct, level int, e0 []int32) []uint64 {
	d := h.Upload(flat)
	defer d.Free()
	de := h.Alloc(len(e0) * 4)
	defer de.Free()
	h.check(C.sfg_memcpy_h2d(h.p, de.Ptr(), unsafe.Pointer(&e0[0]), C.size_t(len(e0)*4)), "h2d")
	dh := h.Alloc(nct * (level + 1) * h.N * 8)
	defer dh.Free()
	h.check(C.sfg_pcks_gen_share_dev(h.p, d.U64(), C.int(nct), C.int(level), (*C.int32_t)(de.Ptr()), nil, dh.U64(), nil), "pcks_gen_share")
	return dh.Download()
}

// PCKSFinishDecode: the local half after the aggregation, fused with the decoding (gwas/gwas.go:385-386): KeySwitch, .Plaintext(), DecodeFloatVector.
func (h *Ctx) PCKSFinishDecode(flat []uint64, nct, level int, scale float64, h0agg []uint64) []float64 {
	d := h.Upload(flat)
	defer d.Free()
	dh := h.Upload(h0agg)
	defer dh.Free()
	out := make([]float64, nct*h.N/2)
	h.check(C.sfg_pcks_finish_decode(h.p, d.U64(), C.int(nct), C.int(level), C.double(scale), dh.U64(), (*C.double)(unsafe.Pointer(&out[0])), nil), "pcks_finish_decode")
	return out
}

// ----------------------------------------------------------------------------------------------------------------
// Secret shares <-> CKKS plaintexts (mpc/ss.go:114-134, 239-279; rvec.hip).  PARITY UNPINNED against the lattigo fork's encoder.EncodeRVecNew / DecodeRVec.
// Field elements are `limbs` little-endian 64-bit words (mpc/ss_hip.go converts); scale is the plaintext's, fracBits mpcObj.GetFracBits().

// EncodeRVec: encoder.EncodeRVecNew (ss.go:125) for nct plaintexts of nElem elements each ([nct][nElem][limbs] words) -> [nct][level+1][N] NTT-domain words.
func (h *Ctx) EncodeRVec(limbs int, modulus, shares []uint64, nElem, nct, level int, scale float64, fracBits int) []uint64 {
	d := h.Upload(shares)
	defer d.Free()
	o := h.Alloc(nct * (level + 1) * h.N * 8)
	defer o.Free()
	h.check(C.sfg_rvec_encode_dev(h.p, C.int(limbs), (*C.uint64_t)(unsafe.Pointer(&modulus[0])), d.U64(), C.int(nElem), C.int(nct), C.int(level), C.double(scale), C.int(fracBits), o.U64()), "rvec_encode")
	return o.Download()
}

// DecodeRVec: encoder.DecodeRVec (ss.go:260,264) of nct plaintexts ([nct][level+1][N] words) -> [nct][nElem][limbs] words.
func (h *Ctx) DecodeRVec(limbs int, modulus, pts []uint64, nct, level int, scale float64, fracBits, nElem int) []uint64 {
	d := h.Upload(pts)
	defer d.Free()
	o := h.Alloc(nct * nElem * limbs * 8)
	defer o.Free()
	h.check(C.sfg_rvec_decode_dev(h.p, C.int(limbs), (*C.uint64_t)(unsafe.Pointer(&modulus[0])), d.U64(), C.size_t((level+1)*h.N), C.int(nct), C.int(level), C.double(scale), C.int(fracBits), C.int(nElem), o.U64()), "rvec_decode")
	return o.Download()
}

// CKKSToSSFinish: ss.go:239-279 after the aggregation - on the hub decode(c0 + h0agg) - decode(maskNTT), elsewhere -decode(maskNTT) (cts and h0agg nil there).
func (h *Ctx) CKKSToSSFinish(limbs int, modulus, cts []uint64, nct, level int, scale float64, fracBits int, h0agg, maskNTT []uint64, isHub bool, nElem int) []uint64 {
	dm := h.Upload(maskNTT)
	defer dm.Free()
	o := h.Alloc(nct * nElem * limbs * 8)
	defer o.Free()
	var pc, ph *C.uint64_t
	hub := 0
	if isHub {
		dc, dh := h.Upload(cts), h.Upload(h0agg)
		defer dc.Free()
		defer dh.Free()
		pc, ph, hub = dc.U64(), dh.U64(), 1
	}
	h.check(C.sfg_ckks_to_ss_finish_dev(h.p, C.int(limbs), (*C.uint64_t)(unsafe.Pointer(&modulus[0])), pc, C.int(nct), C.int(level), C.double(scale), C.int(fracBits), ph, dm.U64(), C.int(hub), C.int(nElem), o.U64()), "ckks_to_ss_finish")
	return o.Download()
}

// ----------------------------------------------------------------------------------------------------------------
// Collective key generation, local halves (mpc/mhe.go:24-105, 381-502; keygen.hip).  PARITY UNPINNED against lattigo's dckks / drlwe protocols.  Shares come back
// as host words for mpc/aggregate.go (AggregatePubKeyShares / AggregateRotKeyShare / AggregateRelinKeyShare sum them modulus by modulus); the aggregated words
// go back in as host words and are installed from device memory.  The errors and the ephemeral secret are drawn on the device from the encryptor's stream
// (SeedEncryptor first); the common reference polynomials come from a seed every party shares (INTEGRATION.md: NOT the bytes of the reference's frand).

// LoadSecretKeyQP gives the device skShard.Value over Q and P (mhe.go:31-46, NTT + Montgomery form); it also serves as LoadSecretKey.
func (h *Ctx) LoadSecretKeyQP(sk *ckks.SecretKey) {
	nmod := h.NQ + h.NP
	flat := make([]uint64, nmod*h.N)
	for m := 0; m < nmod; m++ {
		copy(flat[m*h.N:(m+1)*h.N], sk.Value.Coeffs[m])
	}
	h.check(C.sfg_ctx_load_secret_key_qp(h.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "load_secret_key_qp")
}

// SeedEncryptor keys the device sampler from crypto/rand (what LoadPublicKey does once a public key exists; key generation needs it before).
func (h *Ctx) SeedEncryptor() {
	var key [32]byte
	if _, err := rand.Read(key[:]); err != nil {
		panic(err)
	}
	h.check(C.sfg_ctx_seed_encryptor(h.p, (*C.uint8_t)(unsafe.Pointer(&key[0]))), "seed_encryptor")
	for i := range key {
		key[i] = 0
	}
}

// CommonReferencePolys: crpGen.ReadNew() for npoly consecutive polynomials over Q and P, starting at polynomial firstPoly of the stream under seed32.
func (h *Ctx) CommonReferencePolys(seed32 []byte, firstPoly uint64, npoly int) *DevBuf {
	nmod := h.NQ + h.NP
	mod := make([]int32, npoly*nmod)
	for r := range mod {
		mod[r] = int32(r % nmod)
	}
	d := h.Alloc(npoly * nmod * h.N * 8)
	h.check(C.sfg_crp_fill_dev(h.p, (*C.uint8_t)(unsafe.Pointer(&seed32[0])), C.uint64_t(firstPoly*uint64(nmod)), C.size_t(len(mod)), (*C.int)(unsafe.Pointer(&mod[0])), d.U64()), "crp_fill")
	return d
}

// CollectivePubKeyGenShare: ckgProtocol.GenShare(sk, crp, pkShare) (mhe.go:91).
func (h *Ctx) CollectivePubKeyGenShare(crp *DevBuf) []uint64 {
	d := h.Alloc((h.NQ + h.NP) * h.N * 8)
	defer d.Free()
	h.check(C.sfg_ckg_gen_share_sampled_dev(h.p, crp.U64(), d.U64(), nil), "ckg_gen_share")
	return d.Download()
}

// CollectivePubKeyGenFinish: ckgProtocol.GenPublicKey(pkAgg, crp, pk) (mhe.go:103); the key stays on the device.
func (h *Ctx) CollectivePubKeyGenFinish(agg []uint64, crp *DevBuf) {
	d := h.Upload(agg)
	defer d.Free()
	h.check(C.sfg_ctx_install_public_key_dev(h.p, d.U64(), crp.U64()), "install_public_key")
}

// CollectiveRotKeyGenShares: rtgProtocol.GenShare for a batch of Galois elements (mhe.go:457-465); crp and the result are [len(gElems)][beta][nq+np][N].
func (h *Ctx) CollectiveRotKeyGenShares(gElems []uint64, crp *DevBuf) []uint64 {
	d := h.Alloc(crp.Bytes)
	defer d.Free()
	h.check(C.sfg_rtg_gen_shares_sampled_dev(h.p, (*C.uint64_t)(unsafe.Pointer(&gElems[0])), C.int(len(gElems)), crp.U64(), d.U64(), nil), "rtg_gen_shares")
	return d.Download()
}

// CollectiveRotKeyGenFinish: rtgProtocol.GenRotationKey for the batch (mhe.go:469).
func (h *Ctx) CollectiveRotKeyGenFinish(gElems []uint64, agg []uint64, crp *DevBuf) {
	d := h.Upload(agg)
	defer d.Free()
	h.check(C.sfg_ctx_install_rotkeys_dev(h.p, (*C.uint64_t)(unsafe.Pointer(&gElems[0])), C.int(len(gElems)), d.U64(), crp.U64()), "install_rotkeys")
}

// CollectiveRelinKeyGenRound1: prot.GenShareRoundOne (mhe.go:492); uIndex names the ephemeral secret for round 2 (it is never stored).
func (h *Ctx) CollectiveRelinKeyGenRound1(crp *DevBuf) (h0, h1 []uint64, uIndex uint64) {
	d0, d1 := h.Alloc(crp.Bytes), h.Alloc(crp.Bytes)
	defer d0.Free()
	defer d1.Free()
	var ui C.uint64_t
	h.check(C.sfg_rkg_round1_sampled_dev(h.p, crp.U64(), d0.U64(), d1.U64(), nil, &ui), "rkg_round1")
	return d0.Download(), d1.Download(), uint64(ui)
}

// CollectiveRelinKeyGenRound2: prot.GenShareRoundTwo on the aggregated round-one shares (mhe.go:495).
func (h *Ctx) CollectiveRelinKeyGenRound2(h0agg, h1agg []uint64, uIndex uint64) []uint64 {
	a, b := h.Upload(h0agg), h.Upload(h1agg)
	defer a.Free()
	defer b.Free()
	d := h.Alloc(a.Bytes)
	defer d.Free()
	h.check(C.sfg_rkg_round2_sampled_dev(h.p, a.U64(), b.U64(), C.uint64_t(uIndex), d.U64(), nil), "rkg_round2")
	return d.Download()
}

// CollectiveRelinKeyGenFinish: prot.GenRelinearizationKey(outRound1, outRound2, evk) (mhe.go:498).
func (h *Ctx) CollectiveRelinKeyGenFinish(round2agg, h1agg []uint64) {
	a, b := h.Upload(round2agg), h.Upload(h1agg)
	defer a.Free()
	defer b.Free()
	h.check(C.sfg_ctx_install_relinkey_dev(h.p, a.U64(), b.U64()), "install_relinkey")
}

// mcheck is check for the multi-GPU engine's calls (the failing rank is named in the message).
func (h *Ctx) mcheck(rc C.int, what string) {
	if rc != 0 {
		panic(fmt.Sprintf("sfgwas-hip: %s: %s", what, C.GoString(C.sfg_mgpu_last_error(h.mg))))
	}
}

// Fork returns a handle for another goroutine: same keys and tables, own queues (sfg_ctx_fork).
func (h *Ctx) Fork() *Ctx {
	var c *C.sfg_ctx
	h.check(C.sfg_ctx_fork(h.p, &c), "fork")
	f := *h
	f.p = c
	f.mg = nil // a fork is one caller on devices[0]; the multi-GPU calls belong to the root handle
	return &f
}

// Close destroys the handle (a fork: its queues and scratch; the root: everything, on every device).
func (h *Ctx) Close() {
	if h.mg != nil {
		C.sfg_mgpu_destroy(h.mg) // owns the per-device contexts, h.p among them
		h.mg, h.p = nil, nil
		return
	}
	C.sfg_ctx_destroy(h.p)
	h.p = nil
}

// Raw exposes the C handle to the sibling files of this binding.
func (h *Ctx) Raw() unsafe.Pointer { return unsafe.Pointer(h.p) }

// ----------------------------------------------------------------------------------------------------------------
// Flat layouts.  cgo may read Go memory only for the duration of a call and only if it holds no Go pointers, so the
// [][]uint64 of lattigo polynomials are copied into one []uint64 per call (SURVEY.md §8b "Ownership").

// FlattenSwitchingKey: swk.Value[i][k].Coeffs[m][:] -> [beta][2][nq+np][N] (lattigo keeps these rows in NTT + Montgomery form).
func FlattenSwitchingKey(swk *ckks.SwitchingKey, nmod, n int) []uint64 {
	beta := len(swk.Value)
	flat := make([]uint64, beta*2*nmod*n)
	for i := 0; i < beta; i++ {
		for k := 0; k < 2; k++ {
			for m := 0; m < nmod; m++ {
				copy(flat[((i*2+k)*nmod+m)*n:], swk.Value[i][k].Coeffs[m][:n])
			}
		}
	}
	return flat
}

// CtWords is the number of uint64 words of a degree-1 ciphertext at `level`.
func (h *Ctx) CtWords(level int) int { return 2 * (level + 1) * h.N }

// FlattenCt writes ct.Value()[k].Coeffs[l] for l <= level into dst ([2][level+1][N]); the ciphertext must be at a level >= `level`
// (rows above `level` are dropped: lattigo's DropLevel keeps the first rows).
func (h *Ctx) FlattenCt(ct *ckks.Ciphertext, level int, dst []uint64) {
	nl := level + 1
	for k := 0; k < 2; k++ {
		for l := 0; l < nl; l++ {
			copy(dst[(k*nl+l)*h.N:], ct.Value()[k].Coeffs[l][:h.N])
		}
	}
}

// FlattenVec: a CipherVector ([]*ckks.Ciphertext) at one level, with length-1 broadcasting to n entries.
func (h *Ctx) FlattenVec(v []*ckks.Ciphertext, n, level int) []uint64 {
	w := h.CtWords(level)
	flat := make([]uint64, n*w)
	for i := 0; i < n; i++ {
		src := v[0]
		if len(v) > 1 {
			src = v[i]
		}
		h.FlattenCt(src, level, flat[i*w:(i+1)*w])
	}
	return flat
}

// FlattenCipherMatrix: A[i][b] -> [s][nbr][2][level+1][N].
func (h *Ctx) FlattenCipherMatrix(A [][]*ckks.Ciphertext, level int) []uint64 {
	s, nbr, w := len(A), len(A[0]), h.CtWords(level)
	flat := make([]uint64, s*nbr*w)
	for i := 0; i < s; i++ {
		for b := 0; b < nbr; b++ {
			h.FlattenCt(A[i][b], level, flat[(i*nbr+b)*w:(i*nbr+b+1)*w])
		}
	}
	return flat
}

// CtFromFlat builds a fresh ckks.Ciphertext (the callers mutate results in place, e.g. eval.Sub(out, .., out) at gwas/matmult.go:56,
// so results must be new objects) from [2][level+1][N] words.
func (h *Ctx) CtFromFlat(src []uint64, level int, scale float64) *ckks.Ciphertext {
	ct := ckks.NewCiphertext(h.Params, 1, level, scale)
	nl := level + 1
	for k := 0; k < 2; k++ {
		for l := 0; l < nl; l++ {
			copy(ct.Value()[k].Coeffs[l], src[(k*nl+l)*h.N:(k*nl+l+1)*h.N])
		}
	}
	return ct
}

// VecFromFlat: n ciphertexts from consecutive flat blocks.
func (h *Ctx) VecFromFlat(src []uint64, n, level int, scale float64) []*ckks.Ciphertext {
	w := h.CtWords(level)
	out := make([]*ckks.Ciphertext, n)
	for i := range out {
		out[i] = h.CtFromFlat(src[i*w:(i+1)*w], level, scale)
	}
	return out
}

// AddFlatInto: out[i][j] += ciphertext(flat[i][j]) with lattigo's own Add.  MatMult4Stream / ...Compute start from crypto.CZeroMat - a FRESH
// ENCRYPTION of zero (gwas/matmult.go:1174,1225,1443; crypto/basics.go:367-384) - and add the deterministic sum onto it; the shim
// keeps that, so outputs carry the same fresh randomness the reference's do.
func (h *Ctx) AddFlatInto(eval ckks.Evaluator, out [][]*ckks.Ciphertext, flat []uint64, level int, scale float64) {
	w := h.CtWords(level)
	for i := range out {
		for j := range out[i] {
			k := i*len(out[i]) + j
			ct := h.CtFromFlat(flat[k*w:(k+1)*w], level, scale)
			out[i][j].SetScale(scale) // CZeroMat encrypts at the default scale; the sum carries A.scale * Params.Scale (matmult.go:1045)
			if out[i][j].Level() > level {
				eval.DropLevel(out[i][j], out[i][j].Level()-level)
			}
			eval.Add(out[i][j], ct, out[i][j])
		}
	}
}

// ----------------------------------------------------------------------------------------------------------------
// Device buffers (uint64 words unless stated).

type DevBuf struct {
	h     *Ctx
	p     unsafe.Pointer
	Bytes int
}

func (h *Ctx) Alloc(bytes int) *DevBuf {
	var p unsafe.Pointer
	h.check(C.sfg_malloc(h.p, &p, C.size_t(bytes)), "malloc")
	return &DevBuf{h, p, bytes}
}
func (b *DevBuf) Free()               { b.h.check(C.sfg_free(b.h.p, b.p), "free"); b.p = nil }
func (b *DevBuf) Ptr() unsafe.Pointer { return b.p }
func (b *DevBuf) U64() *C.uint64_t    { return (*C.uint64_t)(b.p) }

// Upload copies host words to a new device buffer.
func (h *Ctx) Upload(words []uint64) *DevBuf {
	b := h.Alloc(8 * len(words))
	h.check(C.sfg_memcpy_h2d(h.p, b.p, unsafe.Pointer(&words[0]), C.size_t(8*len(words))), "h2d")
	return b
}

// Download copies a device buffer back (synchronises the handle's queue; fails while an unprovable encoder rounding is outstanding).
func (b *DevBuf) Download() []uint64 {
	out := make([]uint64, b.Bytes/8)
	b.h.check(C.sfg_memcpy_d2h(b.h.p, unsafe.Pointer(&out[0]), b.p, C.size_t(b.Bytes)), "d2h")
	return out
}

// ----------------------------------------------------------------------------------------------------------------
// Resident genotype matrices, keyed by the reference's cache-file prefix (gwas/pca.go:112-113 passes one prefix for X and one
// for X^T: ONE resident int8 copy serves both, the second prefix is registered with SFG_TRANSPOSE).

type Geno struct {
	g     *C.sfg_geno  // single device
	mg    *C.sfg_mgeno // multi-GPU engine: the matrix sharded by SNP block (exactly one of g / mg is set)
	Flags uint
	NRow  int
	NCol  int
}

// residentGeno is one registered matrix: its handle and stored shape.
type residentGeno struct {
	g          *C.sfg_geno
	mg         *C.sfg_mgeno
	nrow, ncol int
}

var (
	genoMu    sync.Mutex
	genoByKey = map[string]*Geno{}
	resident  []residentGeno // registered matrices, to find X when X^T is registered
)

const (
	FlagSquare    = uint(C.SFG_SQUARE)
	FlagTranspose = uint(C.SFG_TRANSPOSE)
)

// stagingRows is the number of matrix rows one chunk of the row-streamed registration carries: the staging buffer holds
// stagingRows * ncol bytes of page-locked memory (sfg_pinned_alloc), at most stagingBytes - nothing in this package scales with nrow * ncol.
const stagingBytes = 128 << 20

func stagingRows(ncol int) int {
	n := stagingBytes / ncol
	if n < 1 {
		n = 1
	}
	return n
}

// streamRows drives `visit(row0, nrows, chunk)` over the rows that next() yields (GenoFileStream.NextRow, filestream.go:414-426: one row per call, filters
// applied), nrows rows of ncol bytes at a time in a pinned staging buffer.  visit returns false to stop early.
func (h *Ctx) streamRows(nrow, ncol int, next func() []int8, visit func(row0, nrows int, chunk unsafe.Pointer) bool) {
	per := stagingRows(ncol)
	var buf unsafe.Pointer
	h.check(C.sfg_pinned_alloc(h.p, &buf, C.size_t(per*ncol)), "pinned_alloc")
	defer C.sfg_pinned_free(h.p, buf)
	stage := unsafe.Slice((*int8)(buf), per*ncol)
	for row0 := 0; row0 < nrow; row0 += per {
		n := per
		if nrow-row0 < n {
			n = nrow - row0
		}
		for r := 0; r < n; r++ {
			copy(stage[r*ncol:(r+1)*ncol], next())
		}
		if !visit(row0, n, buf) {
			return
		}
	}
}

// RegisterGeno makes the matrix behind a cache prefix resident, reading it the way the reference does - one row at a time (MatMult4StreamPreprocess,
// matmult.go:914-1041: gfs.NextRow per row) - so that no host allocation scales with nrow * ncol.  next() yields the rows in order (filters applied, missing = -1
// kept: the device zeroes negatives before sums and products, matmult.go:1292-1300); reset() rewinds the stream (GenoFileStream.Reset, filestream.go:362-376).
// If the TRANSPOSE of the arriving matrix is already resident (pca.go:112-113 registers X, then X^T from its own file) it is recognised on the device: every
// chunk of arriving rows is compared, entry by entry, with the resident matrix read as its transpose (sfg_geno_compare_rows) - exact, not a hash, and X^T is never
// held anywhere.  The prefix then becomes a SFG_TRANSPOSE view of the one int8 copy.  A shape match with different content (a second, unrelated n x n matrix) falls
// through to a second pass over the stream that uploads it.
func (h *Ctx) RegisterGeno(prefix string, nrow, ncol int, next func() []int8, reset func()) *Geno {
	genoMu.Lock()
	defer genoMu.Unlock()
	if g, ok := genoByKey[prefix]; ok {
		return g
	}
	for _, r := range resident {
		if r.nrow != ncol || r.ncol != nrow {
			continue
		}
		var ndiff C.uint64_t
		reset()
		h.streamRows(nrow, ncol, next, func(row0, n int, chunk unsafe.Pointer) bool {
			if r.mg != nil {
				h.mcheck(C.sfg_mgpu_geno_compare_rows(h.mg, r.mg, C.SFG_TRANSPOSE, C.size_t(row0), C.size_t(n), (*C.int8_t)(chunk), C.size_t(ncol), &ndiff), "mgpu_geno_compare_rows")
			} else {
				h.check(C.sfg_geno_compare_rows(h.p, r.g, C.SFG_TRANSPOSE, C.size_t(row0), C.size_t(n), (*C.int8_t)(chunk), C.size_t(ncol), &ndiff), "geno_compare_rows")
			}
			return ndiff == 0 // the first differing chunk settles it
		})
		if ndiff == 0 {
			e := &Geno{r.g, r.mg, FlagTranspose, nrow, ncol}
			genoByKey[prefix] = e
			return e
		}
	}
	var g *C.sfg_geno
	var m *C.sfg_mgeno
	if h.mg != nil {
		// the STORED orientation is the one whose columns are sharded over the GPUs: pca.go:112-113 registers X (individuals x SNPs) first, so SNP blocks
		// are the shards, Q * X is output-sharded and Q' * X^T contraction-sharded, as SURVEY 8e lays out
		h.mcheck(C.sfg_mgpu_geno_create(h.mg, C.size_t(nrow), C.size_t(ncol), &m), "mgpu_geno_create")
	} else {
		h.check(C.sfg_geno_create(h.p, C.size_t(nrow), C.size_t(ncol), &g), "geno_create")
	}
	reset()
	h.streamRows(nrow, ncol, next, func(row0, n int, chunk unsafe.Pointer) bool {
		if m != nil {
			h.mcheck(C.sfg_mgpu_geno_write_rows(h.mg, m, C.size_t(row0), C.size_t(n), (*C.int8_t)(chunk), C.size_t(ncol)), "mgpu_geno_write_rows")
		} else {
			h.check(C.sfg_geno_write_rows(h.p, g, C.size_t(row0), C.size_t(n), (*C.int8_t)(chunk), C.size_t(ncol)), "geno_write_rows")
		}
		return true
	})
	resident = append(resident, residentGeno{g, m, nrow, ncol})
	e := &Geno{g, m, 0, nrow, ncol}
	genoByKey[prefix] = e
	return e
}

// LookupGeno returns the resident matrix of a prefix, or nil (then MatMult4StreamCompute falls back to the DiagCache files on disk).
func LookupGeno(prefix string) *Geno {
	genoMu.Lock()
	defer genoMu.Unlock()
	return genoByKey[prefix]
}

// ----------------------------------------------------------------------------------------------------------------
// Quality control on a resident matrix (gwas/qualcontrol.go:36-81, 339-378, 416-463; include/sfgwas_hip.h: sfg_geno_qc_scan, sfg_geno_filter).

// QCCounts is what one scan returns, indexed by the matrix's own rows and columns (a dropped row or column holds zeros).
// Col[c][k][j]: kept rows of cohort c (0 = all kept rows, 1 = kept controls) whose call at SNP j is k = 0, 1, 2 or 3 (missing).
type QCCounts struct {
	Col     [2][4][]uint32
	RowMiss []uint32
	RowHet  []uint32
}

func filterPtr(f []bool, n int, store *[]byte) *C.uint8_t {
	if f == nil {
		return nil
	}
	if len(f) != n {
		panic("Invalid length of input array")
	}
	*store = make([]byte, n)
	for i, keep := range f {
		if keep {
			(*store)[i] = 1
		}
	}
	return (*C.uint8_t)(unsafe.Pointer(&(*store)[0]))
}

// QCScan counts, in one pass over the resident matrix, what the three loops of gwas/qualcontrol.go count: rowFilt / colFilt (nil = keep all) say which
// individuals and SNPs are looked at, ctrl (nil = none) marks the control cohort (pheno < 1).  wantCols / wantRows choose the outputs.
// On the multi-GPU engine the row counts are those of this process's ranks.
func (h *Ctx) QCScan(g *Geno, rowFilt, colFilt, ctrl []bool, wantCols, wantRows bool) *QCCounts {
	if g.Flags&FlagTranspose != 0 {
		panic("QCScan: pass the stored matrix (individuals x SNPs), not its transposed view")
	}
	var rs, cs, ts []byte
	pr, pc, pt := filterPtr(rowFilt, g.NRow, &rs), filterPtr(colFilt, g.NCol, &cs), filterPtr(ctrl, g.NRow, &ts)
	out := &QCCounts{}
	var pcol, pmiss, phet *C.uint32_t
	var flat []uint32
	if wantCols {
		flat = make([]uint32, 8*g.NCol)
		pcol = (*C.uint32_t)(unsafe.Pointer(&flat[0]))
		for c := 0; c < 2; c++ {
			for k := 0; k < 4; k++ {
				out.Col[c][k] = flat[(c*4+k)*g.NCol : (c*4+k+1)*g.NCol]
			}
		}
	}
	if wantRows {
		out.RowMiss, out.RowHet = make([]uint32, g.NRow), make([]uint32, g.NRow)
		pmiss, phet = (*C.uint32_t)(unsafe.Pointer(&out.RowMiss[0])), (*C.uint32_t)(unsafe.Pointer(&out.RowHet[0]))
	}
	if g.mg != nil {
		Default.mcheck(C.sfg_mgpu_geno_qc_scan(Default.mg, g.mg, pr, pc, pt, pcol, pmiss, phet), "mgpu_geno_qc_scan")
	} else {
		h.check(C.sfg_geno_qc_scan(h.p, g.g, pr, pc, pt, pcol, pmiss, phet), "geno_qc_scan")
	}
	return out
}

// FilterGeno returns the kept rows and columns of a resident matrix as a new resident matrix (int8 stays int8, packed stays packed):
// FilterMatrixFile (gwas/utilities.go:154) without the files.  A matrix sharded over the multi-GPU engine is re-sharded over the kept SNPs
// (sfg_mgpu_geno_filter): the result multiplies, scans and sketches like any sharded matrix.  The caller registers or frees the result.
func (h *Ctx) FilterGeno(g *Geno, rowFilt, colFilt []bool) *Geno {
	if g.Flags&FlagTranspose != 0 {
		panic("FilterGeno: pass the stored matrix (individuals x SNPs), not its transposed view")
	}
	var rs, cs []byte
	pr, pc := filterPtr(rowFilt, g.NRow, &rs), filterPtr(colFilt, g.NCol, &cs)
	if g.mg != nil {
		var m *C.sfg_mgeno
		Default.mcheck(C.sfg_mgpu_geno_filter(Default.mg, g.mg, pr, pc, &m), "mgpu_geno_filter")
		var mr, mc C.size_t
		C.sfg_mgpu_geno_dims(m, &mr, &mc)
		return &Geno{nil, m, 0, int(mr), int(mc)}
	}
	var f *C.sfg_geno
	h.check(C.sfg_geno_filter(h.p, g.g, pr, pc, &f), "geno_filter")
	var nr, nc C.size_t
	C.sfg_geno_dims(f, &nr, &nc)
	return &Geno{f, nil, 0, int(nr), int(nc)}
}

// FreeGeno returns the device memory of a matrix FilterGeno made (or of any matrix the caller holds unregistered).  g must not be used afterwards.
func (h *Ctx) FreeGeno(g *Geno) {
	if g.mg != nil {
		C.sfg_mgpu_geno_free(Default.mg, g.mg)
	} else if g.g != nil {
		C.sfg_geno_free(h.p, g.g)
	}
	g.g, g.mg = nil, nil
}

// SketchGeno is the plaintext pass of the randomized PCA over the local genotypes (gwas/pca.go:152-162): sketch[k*NCol+j] = sum over the rows i of bucket k of
// sgn[i] * x[i][j] (exact integers in float64), xsum / x2sum the column sums of x and x*x with Go's integer semantics.  On the multi-GPU engine every rank
// sketches its own SNP window (sfg_mgpu_sketch).  A 2-bit packed matrix is refused.
func (h *Ctx) SketchGeno(g *Geno, bucket []int32, sgn []int8, kp int) (sketch []float64, xsum, x2sum []uint64) {
	if g.Flags&FlagTranspose != 0 || len(bucket) != g.NRow || len(sgn) != g.NRow {
		panic("SketchGeno: needs the stored matrix (individuals x SNPs) and one bucket and sign per individual")
	}
	sketch, xsum, x2sum = make([]float64, kp*g.NCol), make([]uint64, g.NCol), make([]uint64, g.NCol)
	pb, ps := (*C.int32_t)(unsafe.Pointer(&bucket[0])), (*C.int8_t)(unsafe.Pointer(&sgn[0]))
	pk, px, px2 := (*C.double)(unsafe.Pointer(&sketch[0])), (*C.uint64_t)(unsafe.Pointer(&xsum[0])), (*C.uint64_t)(unsafe.Pointer(&x2sum[0]))
	if g.mg != nil {
		Default.mcheck(C.sfg_mgpu_sketch(Default.mg, g.mg, pb, ps, C.int(kp), pk, px, px2), "mgpu_sketch")
	} else {
		h.check(C.sfg_sketch(h.p, g.g, pb, ps, C.int(kp), pk, px, px2), "sketch")
	}
	return
}

// ColSumsGeno returns the per-SNP sum and sum of squares after missing -> 0 (gwas/matmult.go:1292-1300); on the multi-GPU engine every rank sums its own
// SNP window (sfg_mgpu_geno_colsums).
func (h *Ctx) ColSumsGeno(g *Geno) (sum, sqsum []float64) {
	if g.Flags&FlagTranspose != 0 {
		panic("ColSumsGeno: pass the stored matrix (individuals x SNPs), not its transposed view")
	}
	sum, sqsum = make([]float64, g.NCol), make([]float64, g.NCol)
	ps, pq := (*C.double)(unsafe.Pointer(&sum[0])), (*C.double)(unsafe.Pointer(&sqsum[0]))
	if g.mg != nil {
		Default.mcheck(C.sfg_mgpu_geno_colsums(Default.mg, g.mg, ps, pq), "mgpu_geno_colsums")
	} else {
		h.check(C.sfg_geno_colsums(h.p, g.g, ps, pq), "geno_colsums")
	}
	return
}

// ----------------------------------------------------------------------------------------------------------------
// The calls the sibling files make.

// MatmulStream = MatMult4Stream on host buffers (include/sfgwas_hip.h: sfg_matmul_stream).
func (h *Ctx) MatmulStream(aFlat []uint64, s, inLevel, maxLevel int, geno []int8, nrow, ncol int, square bool, sum, sqsum []float64) []uint64 {
	mct := (ncol-1)/(h.N/2) + 1
	out := make([]uint64, s*mct*2*maxLevel*h.N)
	flags := C.uint(0)
	if square {
		flags |= C.SFG_SQUARE
	}
	var ps, pq *C.double
	if sum != nil {
		ps, pq = (*C.double)(unsafe.Pointer(&sum[0])), (*C.double)(unsafe.Pointer(&sqsum[0]))
	}
	h.check(C.sfg_matmul_stream(h.p, (*C.uint64_t)(unsafe.Pointer(&aFlat[0])), C.int(s), C.int(inLevel), C.int(maxLevel),
		(*C.int8_t)(unsafe.Pointer(&geno[0])), C.size_t(nrow), C.size_t(ncol), C.size_t(ncol), flags,
		(*C.uint64_t)(unsafe.Pointer(&out[0])), ps, pq), "matmul_stream")
	return out
}

// MatmulResident = MatMult4StreamCompute on a resident matrix; returns [s][m_ct][2][maxLevel][N] words.
func (h *Ctx) MatmulResident(aFlat []uint64, s, inLevel, maxLevel int, g *Geno) []uint64 {
	lcol := g.NCol
	if g.mg != nil { // every GPU of the node: sfg_mgpu_matmul shards, exchanges (Q' * X^T) and gathers
		mctM := (lcol-1)/(h.N/2) + 1
		out := make([]uint64, s*mctM*2*maxLevel*h.N)
		Default.mcheck(C.sfg_mgpu_matmul(Default.mg, (*C.uint64_t)(unsafe.Pointer(&aFlat[0])), C.int(s), C.int(inLevel), C.int(maxLevel), g.mg, C.uint(g.Flags),
			(*C.uint64_t)(unsafe.Pointer(&out[0]))), "mgpu_matmul")
		return out
	}
	dA := h.Upload(aFlat)
	defer dA.Free()
	mct := (lcol-1)/(h.N/2) + 1
	dOut := h.Alloc(8 * s * mct * 2 * maxLevel * h.N)
	defer dOut.Free()
	h.check(C.sfg_matmul_resident_dev(h.p, dA.U64(), C.int(s), C.int(inLevel), C.int(maxLevel), g.g, C.uint(g.Flags), dOut.U64()), "matmul_resident")
	return dOut.Download()
}

// AssocStreamPgen = the per-batch loop of GenoBlockMult's pgen branch (gwas/assoc.go:371-416) for one chromosome file, in one call: per batch of batchSnps kept
// variants FilterMatrixFilePgen + NewGenoFileStream + MatMult4Stream(cps, mat, X, 5, false, square, nproc), the batches' outputs in ConcatCipherMatrix order.
// sampleKeep: one byte per sample of the file (the --keep list of SampleKeepFile), snpFilt: one byte per variant of the file.  The baby-step rotations of `mat`
// are made once for all batches and kept on the device as the int8 MAC's rot tiles (include/sfgwas_hip.h: sfg_assoc_stream_pgen).  Returns [s][nct][2][maxLevel][N]
// words with nct = sum over batches of ceil(kept / slots).
func (h *Ctx) AssocStreamPgen(pgenPath string, sampleKeep, snpFilt []byte, batchSnps int, aFlat []uint64, s, inLevel, maxLevel int, square bool, capacity int) ([]uint64, int) {
	cp := C.CString(pgenPath)
	defer C.free(unsafe.Pointer(cp))
	flags := C.uint(0)
	if square {
		flags |= C.SFG_SQUARE
	}
	var pr, pc *C.uint8_t
	if sampleKeep != nil {
		pr = (*C.uint8_t)(unsafe.Pointer(&sampleKeep[0]))
	}
	if snpFilt != nil {
		pc = (*C.uint8_t)(unsafe.Pointer(&snpFilt[0]))
	}
	var nct C.size_t
	ctw := 2 * maxLevel * h.N
	compact := func(all []uint64) []uint64 { // [s][capacity][ctw] -> [s][nct][ctw]
		out := make([]uint64, s*int(nct)*ctw)
		for i := 0; i < s; i++ {
			copy(out[i*int(nct)*ctw:(i+1)*int(nct)*ctw], all[i*capacity*ctw:(i*capacity+int(nct))*ctw])
		}
		return out
	}
	if h.mg != nil { // batch k on GPU k % G (assoc.go:360-408 hands the batches to assoc_num_blocks_parallel workers the same way)
		nbr := len(aFlat) / (s * 2 * (inLevel + 1) * h.N)
		kept := nbr * (h.N / 2) // A's grid covers the kept samples; the library takes ceil(kept / slots) block rows from this
		all := make([]uint64, s*capacity*ctw)
		h.mcheck(C.sfg_mgpu_assoc_stream_pgen(h.mg, cp, pr, pc, C.size_t(kept), C.size_t(batchSnps), (*C.uint64_t)(unsafe.Pointer(&aFlat[0])), C.int(s), C.int(inLevel),
			C.int(maxLevel), flags, (*C.uint64_t)(unsafe.Pointer(&all[0])), C.size_t(capacity), &nct, nil, nil), "mgpu_assoc_stream_pgen")
		return compact(all), int(nct)
	}
	dA := h.Upload(aFlat)
	defer dA.Free()
	dOut := h.Alloc(8 * s * capacity * 2 * maxLevel * h.N)
	defer dOut.Free()
	h.check(C.sfg_assoc_stream_pgen(h.p, cp, pr, pc, C.size_t(batchSnps), dA.U64(), C.int(s), C.int(inLevel), C.int(maxLevel), flags,
		dOut.U64(), C.size_t(capacity), &nct, nil, nil), "assoc_stream_pgen") // computeSquaredSum = false on this branch (assoc.go:395)
	return compact(dOut.Download()), int(nct) // [s][capacity][2][maxLevel][N]: the first nct ciphertexts of every row
}

// MatmulFromCache = MatMult4StreamCompute on DiagCache files a CPU party wrote (gwas/filestream.go:19-282).
func (h *Ctx) MatmulFromCache(aFlat []uint64, s, inLevel, maxLevel int, prefix string, nbr int) []uint64 {
	cp := C.CString(prefix)
	defer C.free(unsafe.Pointer(cp))
	var hdr [6]C.uint64_t
	h.check(C.sfg_diagcache_header(h.p, cp, 0, &hdr[0]), "diagcache_header")
	mct := int(hdr[0])
	dA := h.Upload(aFlat)
	defer dA.Free()
	dOut := h.Alloc(8 * s * mct * 2 * maxLevel * h.N)
	defer dOut.Free()
	h.check(C.sfg_matmul_from_cache(h.p, dA.U64(), C.int(s), C.int(inLevel), C.int(maxLevel), cp, C.int(nbr), dOut.U64()), "matmul_from_cache")
	return dOut.Download()
}

// RotateRight: a batch of ciphertexts at one level, ct j rotated right by nrot[j] (crypto/basics.go:201-224 semantics).
func (h *Ctx) RotateRight(flat []uint64, nct, level int, nrot []int) []uint64 {
	dIn := h.Upload(flat)
	defer dIn.Free()
	dOut := h.Alloc(8 * len(flat))
	defer dOut.Free()
	cn := make([]C.int, nct)
	for i := range cn {
		cn[i] = C.int(nrot[i])
	}
	h.check(C.sfg_rotate_right_dev(h.p, dIn.U64(), dOut.U64(), C.int(nct), C.int(level), &cn[0]), "rotate_right")
	return dOut.Download()
}

// Binary element-wise ops on equal-level batches: "add", "sub", "mulrelin".
func (h *Ctx) Binary(op string, a, b []uint64, nct, level int) []uint64 {
	dA, dB := h.Upload(a), h.Upload(b)
	defer dA.Free()
	defer dB.Free()
	dOut := h.Alloc(8 * nct * h.CtWords(level))
	defer dOut.Free()
	switch op {
	case "add":
		h.check(C.sfg_ct_add_dev(h.p, dA.U64(), dB.U64(), dOut.U64(), C.int(nct), C.int(level)), op)
	case "sub":
		h.check(C.sfg_ct_sub_dev(h.p, dA.U64(), dB.U64(), dOut.U64(), C.int(nct), C.int(level)), op)
	case "mulrelin":
		h.check(C.sfg_ct_mulrelin_dev(h.p, dA.U64(), dB.U64(), dOut.U64(), C.int(nct), C.int(level)), op)
	default:
		panic("sfgwas-hip: unknown op " + op)
	}
	return dOut.Download()
}

// Rescale divides a batch at `level` by q_level (lattigo DivRoundByLastModulus); output at level-1.
func (h *Ctx) Rescale(in []uint64, nct, level int) []uint64 {
	dIn := h.Upload(in)
	defer dIn.Free()
	dOut := h.Alloc(8 * nct * h.CtWords(level-1))
	defer dOut.Free()
	h.check(C.sfg_ct_rescale_dev(h.p, dIn.U64(), dOut.U64(), C.int(nct), C.int(level)), "rescale")
	return dOut.Download()
}

// InnerSumAll: sum of nct ciphertexts, then the 13 rotate-and-add steps (crypto/basics.go:278-292); one ciphertext out.
func (h *Ctx) InnerSumAll(in []uint64, nct, level int) []uint64 {
	dIn := h.Upload(in)
	defer dIn.Free()
	dOut := h.Alloc(8 * h.CtWords(level))
	defer dOut.Free()
	h.check(C.sfg_ct_innersum_dev(h.p, dIn.U64(), C.int(nct), C.int(level), dOut.U64()), "innersum")
	return dOut.Download()
}

// MulPlain: ciphertext j times NTT-domain plaintext j (eval.MulRelinNew(plaintext, ct) behind crypto.CPMult / Mask, crypto/basics.go:110-172,429-470); one plaintext
// for all when npt == 1.  Level unchanged, the caller multiplies the scales.
func (h *Ctx) MulPlain(cts, pts []uint64, nct, npt, level int) []uint64 {
	dC, dP := h.Upload(cts), h.Upload(pts)
	defer dC.Free()
	defer dP.Free()
	dOut := h.Alloc(8 * nct * h.CtWords(level))
	defer dOut.Free()
	stride := 0
	if npt > 1 {
		stride = (level + 1) * h.N
	}
	h.check(C.sfg_ct_mul_plain_dev(h.p, dC.U64(), dP.U64(), C.size_t(stride), dOut.U64(), C.int(nct), C.int(level)), "mul_plain")
	return dOut.Download()
}

// ----------------------------------------------------------------------------------------------------------------
// Resident ciphertext vectors: the operands of CMult -> MatMult4StreamCompute -> InnerProd (gwas/matmult.go:27-77) stay in HBM between the calls instead of
// crossing PCIe four times.  A DevVec holds Len ciphertexts of ONE level and scale, [Len][2][Level+1][N].

type DevVec struct {
	Buf   *DevBuf
	Len   int
	Level int
	Scale float64
}

func (d *DevVec) Free() { d.Buf.Free() }

// UploadVec: the vector's ciphertexts at their common (minimum) level; their scales must agree (they do for every CipherVector the hot path builds:
// fresh encryptions and bootstrap outputs).
func (h *Ctx) UploadVec(v []*ckks.Ciphertext) *DevVec {
	level, scale := v[0].Level(), v[0].Scale()
	for _, c := range v {
		if c.Level() < level {
			level = c.Level()
		}
		if c.Scale() != scale {
			panic("sfgwas-hip: UploadVec: ciphertexts of one vector at different scales")
		}
	}
	return &DevVec{h.Upload(h.FlattenVec(v, len(v), level)), len(v), level, scale}
}

// DownloadVec: fresh ckks.Ciphertexts.
func (h *Ctx) DownloadVec(d *DevVec) []*ckks.Ciphertext {
	return h.VecFromFlat(d.Buf.Download(), d.Len, d.Level, d.Scale)
}

// dropTo returns a view of d at `level` (a new buffer when rows have to go: DropLevel keeps the first level + 1 rows of either polynomial).
func (h *Ctx) dropTo(d *DevVec, level int) (*DevVec, bool) {
	if d.Level == level {
		return d, false
	}
	out := h.Alloc(8 * d.Len * h.CtWords(level))
	h.check(C.sfg_ct_drop_level_dev(h.p, d.Buf.U64(), out.U64(), C.int(d.Len), C.int(d.Level), C.int(level)), "drop_level")
	return &DevVec{out, d.Len, level, d.Scale}, true
}

// CMultDev = crypto.CMult (crypto/basics.go:386-427) on resident operands: MulRelinNew + Rescale(minScale) per ciphertext, b broadcast when b.Len == 1.
// Every entry of a DevVec shares level and scale, so the whole vector is one (level, scale) group.
func (h *Ctx) CMultDev(a, b *DevVec, minScale float64) *DevVec {
	level := a.Level
	if b.Level < level {
		level = b.Level
	}
	n := a.Len
	if b.Len > n {
		n = b.Len
	}
	x, fx := h.dropTo(a, level)
	y, fy := h.dropTo(b, level)
	w := h.CtWords(level)
	rep := func(v *DevVec) *DevBuf { // length-1 broadcasting: n copies on the device
		if v.Len == n {
			return v.Buf
		}
		r := h.Alloc(8 * n * w)
		for i := 0; i < n; i++ {
			h.check(C.sfg_memcpy_d2d(h.p, unsafe.Pointer(uintptr(r.p)+uintptr(8*i*w)), v.Buf.p, C.size_t(8*w)), "d2d")
		}
		return r
	}
	bx, by := rep(x), rep(y)
	out := h.Alloc(8 * n * w)
	h.check(C.sfg_ct_mulrelin_dev(h.p, bx.U64(), by.U64(), out.U64(), C.int(n), C.int(level)), "mulrelin")
	if bx != x.Buf {
		bx.Free()
	}
	if by != y.Buf {
		by.Free()
	}
	if fx {
		x.Free()
	}
	if fy {
		y.Free()
	}
	scale := a.Scale * b.Scale
	qi := h.Params.Qi()
	for level > 0 && scale/float64(qi[level]) >= minScale/2 { // ckks.Evaluator.Rescale's loop (threshold scale)
		nxt := h.Alloc(8 * n * h.CtWords(level-1))
		h.check(C.sfg_ct_rescale_dev(h.p, out.U64(), nxt.U64(), C.int(n), C.int(level)), "rescale")
		out.Free()
		out = nxt
		scale /= float64(qi[level])
		level--
	}
	return &DevVec{out, n, level, scale}
}

// InnerSumAllDev = crypto.InnerSumAll (crypto/basics.go:278-292) on a resident vector: one ciphertext, the total in every slot.
func (h *Ctx) InnerSumAllDev(a *DevVec) *DevVec {
	out := h.Alloc(8 * h.CtWords(a.Level))
	h.check(C.sfg_ct_innersum_dev(h.p, a.Buf.U64(), C.int(a.Len), C.int(a.Level), out.U64()), "innersum")
	return &DevVec{out, 1, a.Level, a.Scale}
}

// MatmulResidentRows = MatMult4StreamCompute with the rows of A resident (each a DevVec of nbr ciphertexts at one common level): on a single device the input grid is
// assembled by device copies; with the multi-GPU engine the rows are downloaded once and the engine shards them.  Returns [s][m_ct][2][maxLevel][N] words.
func (h *Ctx) MatmulResidentRows(rows []*DevVec, maxLevel int, g *Geno) []uint64 {
	s, nbr, level := len(rows), rows[0].Len, rows[0].Level
	for _, r := range rows {
		if r.Len != nbr || r.Level != level {
			panic("sfgwas-hip: MatmulResidentRows: rows of different shape")
		}
	}
	w := h.CtWords(level)
	if g.mg != nil {
		flat := make([]uint64, s*nbr*w)
		for i, r := range rows {
			copy(flat[i*nbr*w:], r.Buf.Download())
		}
		return h.MatmulResident(flat, s, level, maxLevel, g)
	}
	grid := h.Alloc(8 * s * nbr * w)
	defer grid.Free()
	for i, r := range rows {
		h.check(C.sfg_memcpy_d2d(h.p, unsafe.Pointer(uintptr(grid.p)+uintptr(8*i*nbr*w)), r.Buf.p, C.size_t(8*nbr*w)), "d2d")
	}
	mct := (g.NCol-1)/(h.N/2) + 1
	dOut := h.Alloc(8 * s * mct * 2 * maxLevel * h.N)
	defer dOut.Free()
	h.check(C.sfg_matmul_resident_dev(h.p, grid.U64(), C.int(s), C.int(level), C.int(maxLevel), g.g, C.uint(g.Flags), dOut.U64()), "matmul_resident")
	return dOut.Download()
}

// BeaverElem / BeaverMatmul: local Beaver products over a prime field of `limbs` 64-bit little-endian limbs (mpc/beavermult.go:94-147).
func (h *Ctx) BeaverElem(pid, limbs int, modulus, ar, am, br, bm []uint64, n int) []uint64 {
	out := make([]uint64, n*limbs)
	p := func(s []uint64) *C.uint64_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.uint64_t)(unsafe.Pointer(&s[0]))
	}
	h.check(C.sfg_beaver_elem(h.p, C.int(pid), C.int(limbs), p(modulus), p(ar), p(am), p(br), p(bm), p(out), C.size_t(n)), "beaver_elem")
	return out
}
func (h *Ctx) BeaverMatmul(pid, limbs int, modulus, ar, am, br, bm []uint64, m, k, n int) []uint64 {
	out := make([]uint64, m*n*limbs)
	p := func(s []uint64) *C.uint64_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.uint64_t)(unsafe.Pointer(&s[0]))
	}
	h.check(C.sfg_beaver_matmul(h.p, C.int(pid), C.int(limbs), p(modulus), p(ar), p(am), p(br), p(bm), p(out), C.int(m), C.int(k), C.int(n)), "beaver_matmul")
	return out
}

// ----------------------------------------------------------------------------------------------------------------
// The general ring: the evaluator operations of crypto/basics.go at the presets the specialised context does not serve (gwas/gwas.go:164-177: PN12QP109,
// PN13QP218, PN15QP880, PN16QP1761 - any logN 12..16 with prime moduli below 2^61), its two ends, its collective key generation and bootstrap, and the two matrix
// products (INTEGRATION.md, "The other CKKS presets").  A Ring keeps Ctx's host-side conventions: flat [nct][2][level+1][N] words in and out, panics on failure.
type Ring struct {
	p      *C.sfg_ring
	Params *ckks.Parameters
	N      int
	NQ, NP int
}

// DefaultRing is set by InitRing; gwas.go calls InitRing instead of Init when config.CkksParams is not "PN14QP438".
var DefaultRing *Ring

// Evaluator is what the drop-in bodies of crypto/basics_hip.go need of a device evaluator; *Ctx and *Ring both provide it.
type Evaluator interface {
	Degree() int
	Parameters() *ckks.Parameters
	CtWords(level int) int
	FlattenCt(ct *ckks.Ciphertext, level int, dst []uint64)
	FlattenVec(v []*ckks.Ciphertext, n, level int) []uint64
	CtFromFlat(src []uint64, level int, scale float64) *ckks.Ciphertext
	VecFromFlat(src []uint64, n, level int, scale float64) []*ckks.Ciphertext
	RotateRight(flat []uint64, nct, level int, nrot []int) []uint64
	Binary(op string, a, b []uint64, nct, level int) []uint64
	Rescale(in []uint64, nct, level int) []uint64
	InnerSumAll(in []uint64, nct, level int) []uint64
	MulPlain(cts, pts []uint64, nct, npt, level int) []uint64
}

// For returns the device evaluator of the process: the general ring when InitRing made one (a preset other than PN14QP438), else the specialised context.
func For(params *ckks.Parameters) Evaluator {
	if DefaultRing != nil && DefaultRing.Params == params {
		return DefaultRing
	}
	return Default
}

func (h *Ctx) Degree() int                   { return h.N }
func (h *Ctx) Parameters() *ckks.Parameters  { return h.Params }
func (r *Ring) Degree() int                  { return r.N }
func (r *Ring) Parameters() *ckks.Parameters { return r.Params }

func (r *Ring) check(rc C.int, what string) {
	if rc != 0 {
		panic(fmt.Sprintf("sfgwas-hip: %s: %s", what, C.GoString(C.sfg_ring_last_error(r.p))))
	}
}

// InitRing creates the general ring from the CKKS parameters (lattigo's own moduli and 2N-th roots) and uploads the switching keys the party holds.
func InitRing(params *ckks.Parameters, rotKs *ckks.RotationKeySet, rlk *ckks.RelinearizationKey, device int) *Ring {
	qi, pi := params.Qi(), params.Pi()
	moduli := append(append([]uint64{}, qi...), pi...)
	ringQP, err := ring.NewRing(params.N(), moduli)
	if err != nil {
		panic(err)
	}
	psi := make([]uint64, len(moduli))
	for i := range moduli {
		psi[i] = ring.InvMForm(ringQP.PsiMont[i], moduli[i], ringQP.MredParams[i])
	}
	r := &Ring{Params: params, N: params.N(), NQ: len(qi), NP: len(pi)}
	if C.sfg_ring_create(&r.p, C.int(device), C.int(params.LogN()), C.int(len(qi)), C.int(len(pi)),
		(*C.uint64_t)(unsafe.Pointer(&moduli[0])), (*C.uint64_t)(unsafe.Pointer(&psi[0]))) != 0 {
		panic("sfgwas-hip: sfg_ring_create: " + C.GoString(C.sfg_ring_last_error(nil)))
	}
	if rotKs != nil {
		for galEl, swk := range rotKs.Keys {
			r.LoadRotKey(galEl, swk)
		}
	}
	if rlk != nil && len(rlk.Keys) > 0 {
		r.LoadRelinKey(rlk.Keys[0])
	}
	DefaultRing = r
	return r
}

func (r *Ring) Close() {
	if r.p != nil {
		C.sfg_ring_destroy(r.p)
		r.p = nil
	}
	if DefaultRing == r {
		DefaultRing = nil
	}
}

func (r *Ring) Sync() { r.check(C.sfg_ring_synchronize(r.p), "ring_synchronize") }

// LoadRotKey / LoadRelinKey: lattigo's switching keys, flattened to [beta][2][nq+np][N], in their stored Montgomery form.
func (r *Ring) LoadRotKey(galEl uint64, swk *ckks.SwitchingKey) {
	flat := FlattenSwitchingKey(swk, r.NQ+r.NP, r.N)
	r.check(C.sfg_ring_load_rotkey(r.p, C.uint64_t(galEl), (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "ring_load_rotkey")
}
func (r *Ring) HasRotKey(galEl uint64) bool { return C.sfg_ring_has_rotkey(r.p, C.uint64_t(galEl)) != 0 }
func (r *Ring) LoadRelinKey(swk *ckks.SwitchingKey) {
	flat := FlattenSwitchingKey(swk, r.NQ+r.NP, r.N)
	r.check(C.sfg_ring_load_relinkey(r.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "ring_load_relinkey")
}
func (r *Ring) GaloisForRotation(kLeft int) uint64 {
	return uint64(C.sfg_ring_galois_for_rotation(r.p, C.int(kLeft)))
}

// device memory of the ring
func (r *Ring) alloc(words int) *C.uint64_t {
	var p unsafe.Pointer
	r.check(C.sfg_ring_malloc(r.p, &p, C.size_t(8*words)), "ring_malloc")
	return (*C.uint64_t)(p)
}
func (r *Ring) free(p *C.uint64_t) { r.check(C.sfg_ring_free(r.p, unsafe.Pointer(p)), "ring_free") }
func (r *Ring) upload(words []uint64) *C.uint64_t {
	p := r.alloc(len(words))
	r.check(C.sfg_ring_memcpy_h2d(r.p, unsafe.Pointer(p), unsafe.Pointer(&words[0]), C.size_t(8*len(words))), "ring_memcpy_h2d")
	return p
}
func (r *Ring) download(p *C.uint64_t, words int) []uint64 {
	out := make([]uint64, words)
	r.check(C.sfg_ring_memcpy_d2h(r.p, unsafe.Pointer(&out[0]), unsafe.Pointer(p), C.size_t(8*words)), "ring_memcpy_d2h")
	return out
}

// the flat-layout helpers are Ctx's own, on the ring's parameters
func (r *Ring) host() *Ctx           { return &Ctx{Params: r.Params, N: r.N, NQ: r.NQ, NP: r.NP} }
func (r *Ring) CtWords(level int) int { return 2 * (level + 1) * r.N }
func (r *Ring) FlattenCt(ct *ckks.Ciphertext, level int, dst []uint64) {
	r.host().FlattenCt(ct, level, dst)
}
func (r *Ring) FlattenVec(v []*ckks.Ciphertext, n, level int) []uint64 {
	return r.host().FlattenVec(v, n, level)
}
func (r *Ring) CtFromFlat(src []uint64, level int, scale float64) *ckks.Ciphertext {
	return r.host().CtFromFlat(src, level, scale)
}
func (r *Ring) VecFromFlat(src []uint64, n, level int, scale float64) []*ckks.Ciphertext {
	return r.host().VecFromFlat(src, n, level, scale)
}

// unary runs one call that maps a batch at `level` to a batch of outWords words
func (r *Ring) unary(in []uint64, outWords int, what string, call func(dIn, dOut *C.uint64_t) C.int) []uint64 {
	dIn := r.upload(in)
	defer r.free(dIn)
	dOut := r.alloc(outWords)
	defer r.free(dOut)
	r.check(call(dIn, dOut), what)
	return r.download(dOut, outWords)
}

// NTTRows / INTTRows: rows of N words, row i modulo moduli[modIdx[i]] (lattigo ring.NTT / ring.InvNTT).
func (r *Ring) NTTRows(rows []uint64, modIdx []int) []uint64 {
	mi := make([]C.int, len(modIdx))
	for i := range mi {
		mi[i] = C.int(modIdx[i])
	}
	d := r.upload(rows)
	defer r.free(d)
	r.check(C.sfg_ring_ntt_rows(r.p, d, C.int(len(mi)), &mi[0]), "ring_ntt_rows")
	return r.download(d, len(rows))
}
func (r *Ring) INTTRows(rows []uint64, modIdx []int) []uint64 {
	mi := make([]C.int, len(modIdx))
	for i := range mi {
		mi[i] = C.int(modIdx[i])
	}
	d := r.upload(rows)
	defer r.free(d)
	r.check(C.sfg_ring_intt_rows(r.p, d, C.int(len(mi)), &mi[0]), "ring_intt_rows")
	return r.download(d, len(rows))
}

// RotateRight - crypto/basics.go:201-224 on a batch: ct j rotated right by nrot[j].
func (r *Ring) RotateRight(flat []uint64, nct, level int, nrot []int) []uint64 {
	cn := make([]C.int, nct)
	for i := range cn {
		cn[i] = C.int(nrot[i])
	}
	return r.unary(flat, len(flat), "ring_rotate_right", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_rotate_right_dev(r.p, dIn, dOut, C.int(nct), C.int(level), &cn[0])
	})
}

// Galois - eval.ConjugateNew (galEl = 2N-1) and any other automorphism whose key is loaded (crypto/basics.go:826-846).
func (r *Ring) Galois(flat []uint64, nct, level int, galEl uint64) []uint64 {
	return r.unary(flat, len(flat), "ring_ct_galois", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_galois_dev(r.p, dIn, dOut, C.int(nct), C.int(level), C.uint64_t(galEl))
	})
}

// Binary element-wise ops on equal-level batches: "add", "sub", "mulrelin".
func (r *Ring) Binary(op string, a, b []uint64, nct, level int) []uint64 {
	dB := r.upload(b)
	defer r.free(dB)
	return r.unary(a, nct*r.CtWords(level), "ring_"+op, func(dA, dOut *C.uint64_t) C.int {
		switch op {
		case "add":
			return C.sfg_ring_ct_add_dev(r.p, dA, dB, dOut, C.int(nct), C.int(level))
		case "sub":
			return C.sfg_ring_ct_sub_dev(r.p, dA, dB, dOut, C.int(nct), C.int(level))
		case "mulrelin":
			return C.sfg_ring_ct_mulrelin_dev(r.p, dA, dB, dOut, C.int(nct), C.int(level))
		}
		panic("sfgwas-hip: unknown op " + op)
	})
}

// DropLevel - crypto.DropLevel (crypto/basics.go:806-824).
func (r *Ring) DropLevel(in []uint64, nct, levelIn, levelOut int) []uint64 {
	return r.unary(in, nct*r.CtWords(levelOut), "ring_ct_drop_level", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_drop_level_dev(r.p, dIn, dOut, C.int(nct), C.int(levelIn), C.int(levelOut))
	})
}

// MulScalar / AddScalar / MulScalarAdd: one canonical residue per modulus (lattigo's scaleUpExact and the scale bookkeeping stay with the caller, as for Ctx).
func (r *Ring) MulScalar(in, scalars []uint64, nct, level int) []uint64 {
	return r.unary(in, len(in), "ring_ct_mul_scalar", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_mul_scalar_dev(r.p, dIn, (*C.uint64_t)(unsafe.Pointer(&scalars[0])), dOut, C.int(nct), C.int(level))
	})
}
func (r *Ring) AddScalar(in, scalars []uint64, nct, level int) []uint64 {
	return r.unary(in, len(in), "ring_ct_add_scalar", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_add_scalar_dev(r.p, dIn, (*C.uint64_t)(unsafe.Pointer(&scalars[0])), dOut, C.int(nct), C.int(level))
	})
}
func (r *Ring) MulScalarAdd(in, scalars, acc []uint64, nct, level int) []uint64 {
	dIn, dAcc := r.upload(in), r.upload(acc)
	defer r.free(dIn)
	defer r.free(dAcc)
	r.check(C.sfg_ring_ct_mul_scalar_add_dev(r.p, dIn, (*C.uint64_t)(unsafe.Pointer(&scalars[0])), dAcc, C.int(nct), C.int(level)), "ring_ct_mul_scalar_add")
	return r.download(dAcc, len(acc))
}

// AddPlain / MulPlain: ciphertext j and NTT-domain plaintext j; one plaintext for all when npt == 1 (crypto/basics.go:110-172, 183-190, 429-470, 592-602).
func (r *Ring) AddPlain(cts, pts []uint64, nct, npt, level int) []uint64 {
	dP := r.upload(pts)
	defer r.free(dP)
	stride := 0
	if npt > 1 {
		stride = (level + 1) * r.N
	}
	return r.unary(cts, len(cts), "ring_ct_add_plain", func(dC, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_add_plain_dev(r.p, dC, dP, C.size_t(stride), dOut, C.int(nct), C.int(level))
	})
}
func (r *Ring) MulPlain(cts, pts []uint64, nct, npt, level int) []uint64 {
	dP := r.upload(pts)
	defer r.free(dP)
	stride := 0
	if npt > 1 {
		stride = (level + 1) * r.N
	}
	return r.unary(cts, len(cts), "ring_ct_mul_plain", func(dC, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_mul_plain_dev(r.p, dC, dP, C.size_t(stride), dOut, C.int(nct), C.int(level))
	})
}

// Rescale divides a batch at `level` by q_level; output at level-1.
func (r *Ring) Rescale(in []uint64, nct, level int) []uint64 {
	return r.unary(in, nct*r.CtWords(level-1), "ring_ct_rescale", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_rescale_dev(r.p, dIn, dOut, C.int(nct), C.int(level))
	})
}

// InnerSumAll: sum of nct ciphertexts, then the log2(slots) rotate-and-add steps (crypto/basics.go:278-292); one ciphertext out.
func (r *Ring) InnerSumAll(in []uint64, nct, level int) []uint64 {
	return r.unary(in, r.CtWords(level), "ring_ct_innersum", func(dIn, dOut *C.uint64_t) C.int {
		return C.sfg_ring_ct_innersum_dev(r.p, dIn, C.int(nct), C.int(level), dOut)
	})
}

// ---- the ring's two ends (gring_io.hip): the encoder, public-key encryption, the collective decryption's local halves, decryption and the decoder.

// LoadPublicKey gives the ring cryptoParams.Pk (crypto/crypto.go:45, Montgomery form) and keys the device sampler from crypto/rand, as Ctx.LoadPublicKey does.
func (r *Ring) LoadPublicKey(pk *ckks.PublicKey) {
	nmod := r.NQ + r.NP
	flat := make([]uint64, 2*nmod*r.N)
	for k := 0; k < 2; k++ {
		for m := 0; m < nmod; m++ {
			copy(flat[(k*nmod+m)*r.N:(k*nmod+m+1)*r.N], pk.Value[k].Coeffs[m])
		}
	}
	r.check(C.sfg_ring_load_public_key(r.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "ring_load_public_key")
	r.SeedEncryptor()
}
func (r *Ring) allocBytes(n int) unsafe.Pointer {
	var p unsafe.Pointer
	r.check(C.sfg_ring_malloc(r.p, &p, C.size_t(n)), "ring_malloc")
	return p
}
func (r *Ring) freeBytes(p unsafe.Pointer) { r.check(C.sfg_ring_free(r.p, p), "ring_free") }
func (r *Ring) HasPublicKey() bool { return C.sfg_ring_has_public_key(r.p) != 0 }

// SeedEncryptor keys the ring's sampler from crypto/rand; the key is wiped from this process's memory after the call.
func (r *Ring) SeedEncryptor() {
	var key [32]byte
	if _, err := rand.Read(key[:]); err != nil {
		panic(err)
	}
	r.check(C.sfg_ring_seed_encryptor(r.p, (*C.uint8_t)(unsafe.Pointer(&key[0]))), "ring_seed_encryptor")
	for i := range key {
		key[i] = 0
	}
}
func (r *Ring) EncryptorNextIndex() uint64 {
	var n C.uint64_t
	r.check(C.sfg_ring_encryptor_next_index(r.p, &n), "ring_encryptor_next_index")
	return uint64(n)
}

// LoadSecretKey gives the ring cryptoParams.Sk (crypto/crypto.go:44, NTT + Montgomery form): this party's shard for PCKSGenShare.
func (r *Ring) LoadSecretKey(sk *ckks.SecretKey) {
	flat := make([]uint64, r.NQ*r.N)
	for m := 0; m < r.NQ; m++ {
		copy(flat[m*r.N:(m+1)*r.N], sk.Value.Coeffs[m])
	}
	r.check(C.sfg_ring_load_secret_key(r.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "ring_load_secret_key")
}

// EncodeVectors: encoder.Encode of nvec real slot vectors ([nvec][N/2] doubles) at `scale` -> NTT-domain plaintext rows [nvec][level+1][N] (every coefficient the
// exactly rounded integer, or the call fails).
func (r *Ring) EncodeVectors(values []float64, nvec, level int, scale float64) []uint64 {
	words := nvec * (level + 1) * r.N
	d := r.alloc(words)
	defer r.free(d)
	r.check(C.sfg_ring_encode_vectors_dev(r.p, (*C.double)(unsafe.Pointer(&values[0])), C.int(nvec), C.int(level), C.double(scale), d), "ring_encode_vectors")
	return r.download(d, words)
}

// EncryptFloatVector: crypto.EncryptFloatVector (crypto.go:340-362) - f packed into ceil(len/slots) ciphertexts at `level` and the parameters' default scale, encoded
// and encrypted on the device; only the doubles go up.
func (r *Ring) EncryptFloatVector(f []float64, level int) []*ckks.Ciphertext {
	slots := r.N / 2
	nvec := (len(f) + slots - 1) / slots
	padded := make([]float64, nvec*slots)
	copy(padded, f)
	words := nvec * r.CtWords(level)
	d := r.alloc(words)
	defer r.free(d)
	r.check(C.sfg_ring_encrypt_vectors_dev(r.p, (*C.double)(unsafe.Pointer(&padded[0])), C.int(nvec), C.int(level), C.double(r.Params.Scale()), d), "ring_encrypt_vectors")
	return r.VecFromFlat(r.download(d, words), nvec, level, r.Params.Scale())
}

// Zeros: crypto.CZeros (basics.go:367-384) - n fresh encryptions of zero: ct += Enc(0) on zeroed words.
func (r *Ring) Zeros(n, level int) []uint64 {
	return r.AddFreshZero(make([]uint64, n*r.CtWords(level)), n, level)
}

// EncryptExplicit: the deterministic core on the caller's samples (u in {-1, 0, 1}, e0, e1 small), pts nil or [nct][level+1][N].
func (r *Ring) EncryptExplicit(pts []uint64, nct, level int, u []int8, e0, e1 []int32) []uint64 {
	var dPt *C.uint64_t
	if pts != nil {
		dPt = r.upload(pts)
		defer r.free(dPt)
	}
	du, d0, d1 := r.allocBytes(len(u)), r.allocBytes(4*len(e0)), r.allocBytes(4*len(e1))
	defer r.freeBytes(du)
	defer r.freeBytes(d0)
	defer r.freeBytes(d1)
	r.check(C.sfg_ring_memcpy_h2d(r.p, du, unsafe.Pointer(&u[0]), C.size_t(len(u))), "ring_memcpy_h2d")
	r.check(C.sfg_ring_memcpy_h2d(r.p, d0, unsafe.Pointer(&e0[0]), C.size_t(4*len(e0))), "ring_memcpy_h2d")
	r.check(C.sfg_ring_memcpy_h2d(r.p, d1, unsafe.Pointer(&e1[0]), C.size_t(4*len(e1))), "ring_memcpy_h2d")
	dOut := r.alloc(nct * r.CtWords(level))
	defer r.free(dOut)
	r.check(C.sfg_ring_encrypt_explicit_dev(r.p, dPt, C.int(nct), C.int(level), (*C.int8_t)(du), (*C.int32_t)(d0), (*C.int32_t)(d1), dOut), "ring_encrypt_explicit")
	return r.download(dOut, nct*r.CtWords(level))
}

// AddFreshZero: crypto.CZeroMat + eval.Add (matmult.go:1174,1225,1443,1494): every ciphertext += a fresh encryption of zero.
func (r *Ring) AddFreshZero(flat []uint64, nct, level int) []uint64 {
	d := r.upload(flat)
	defer r.free(d)
	r.check(C.sfg_ring_ct_add_fresh_zero_dev(r.p, d, C.int(nct), C.int(level)), "ring_ct_add_fresh_zero")
	return r.download(d, len(flat))
}

// PCKSGenShare: the local half of CollectiveDecrypt* before the aggregation (mpc/mhe.go:107-220): h0 [nct][level+1][N] from this party's key shard and its own
// error polynomials e0 [nct][N] (sigma 6.36, bound 38 in the reference); polynomial 1 of the share is not computed (the reference discards it).
func (r *Ring) PCKSGenShare(flat []uint64, nct, level int, e0 []int32) []uint64 {
	d := r.upload(flat)
	defer r.free(d)
	de := r.allocBytes(4 * len(e0))
	defer r.freeBytes(de)
	r.check(C.sfg_ring_memcpy_h2d(r.p, de, unsafe.Pointer(&e0[0]), C.size_t(4*len(e0))), "ring_memcpy_h2d")
	dh := r.alloc(nct * (level + 1) * r.N)
	defer r.free(dh)
	r.check(C.sfg_ring_pcks_gen_share_dev(r.p, d, C.int(nct), C.int(level), (*C.int32_t)(de), nil, dh, nil), "ring_pcks_gen_share")
	return r.download(dh, nct*(level+1)*r.N)
}

// PCKSFinish: the local half after the aggregation: the plaintext rows [nct][level+1][N] = c0 + h0agg, for lattigo's encoder.Decode.
func (r *Ring) PCKSFinish(flat []uint64, nct, level int, h0agg []uint64) []uint64 {
	d := r.upload(flat)
	defer r.free(d)
	dh := r.upload(h0agg)
	defer r.free(dh)
	dOut := r.alloc(nct * (level + 1) * r.N)
	defer r.free(dOut)
	r.check(C.sfg_ring_pcks_finish_dev(r.p, d, C.int(nct), C.int(level), dh, dOut), "ring_pcks_finish")
	return r.download(dOut, nct*(level+1)*r.N)
}

// RefreshGenShares: the local half of BootstrapMatAll / CollectiveBootstrapMat / CollectiveBootstrapVec before the aggregation (mpc/mhe.go:251,315:
// refProtocol.GenShares(skShard, levelStart, nParties, ct, parameters.Scale(), crp, ...)) for nct ciphertexts of one level: h0 [nct][level+1][N] and
// h1 [nct][nq][N] from this party's key shard, its masks ([nct][N][maskLimbs] two's-complement limbs, ring.RandInt below Q_level / (2 nParties) recentred), its
// error polynomials e0, e1 [nct][N] and the common reference polynomials crs [nct][nq][N].  ctScale is the scale the ciphertexts carry, the target is always
// Params.Scale(), as the reference passes it.  PARITY UNPINNED (see include/sfgwas_hip.h).
func (r *Ring) RefreshGenShares(flat []uint64, nct, level int, ctScale float64, crs, masks []uint64, maskLimbs int, e0, e1 []int32) (h0, h1 []uint64) {
	d, dc, dm := r.upload(flat), r.upload(crs), r.upload(masks)
	defer r.free(d)
	defer r.free(dc)
	defer r.free(dm)
	d0, d1 := r.allocBytes(4*len(e0)), r.allocBytes(4*len(e1))
	defer r.freeBytes(d0)
	defer r.freeBytes(d1)
	r.check(C.sfg_ring_memcpy_h2d(r.p, d0, unsafe.Pointer(&e0[0]), C.size_t(4*len(e0))), "ring_memcpy_h2d")
	r.check(C.sfg_ring_memcpy_h2d(r.p, d1, unsafe.Pointer(&e1[0]), C.size_t(4*len(e1))), "ring_memcpy_h2d")
	dh0, dh1 := r.alloc(nct*(level+1)*r.N), r.alloc(nct*r.NQ*r.N)
	defer r.free(dh0)
	defer r.free(dh1)
	r.check(C.sfg_ring_refresh_gen_shares_scaled_dev(r.p, d, C.int(nct), C.int(level), C.double(ctScale), C.double(r.Params.Scale()), dc, dm, C.int(maskLimbs),
		(*C.int32_t)(d0), (*C.int32_t)(d1), dh0, dh1), "ring_refresh_gen_shares")
	return r.download(dh0, nct*(level+1)*r.N), r.download(dh1, nct*r.NQ*r.N)
}

// RefreshFinish: the local half after the aggregation (mpc/mhe.go:256-258,329-331: Decrypt, Recode(ct, parameters.Scale()), Recrypt): the refreshed ciphertexts
// [nct][2][nq][N] at level nq - 1 and scale Params.Scale() from the aggregated shares h0agg [nct][level+1][N], h1agg [nct][nq][N] and crs.
func (r *Ring) RefreshFinish(flat []uint64, nct, level int, ctScale float64, h0agg, h1agg, crs []uint64) []uint64 {
	d, d0, d1, dc := r.upload(flat), r.upload(h0agg), r.upload(h1agg), r.upload(crs)
	defer r.free(d)
	defer r.free(d0)
	defer r.free(d1)
	defer r.free(dc)
	dOut := r.alloc(nct * 2 * r.NQ * r.N)
	defer r.free(dOut)
	r.check(C.sfg_ring_refresh_finish_scaled_dev(r.p, d, C.int(nct), C.int(level), C.double(ctScale), C.double(r.Params.Scale()), d0, d1, dc, dOut), "ring_refresh_finish")
	return r.download(dOut, nct*2*r.NQ*r.N)
}

// DecodeCoeffs: the first half of crypto.DecodeFloatVector (crypto.go:525-536 -> encoder.Decode) for nvec NTT-domain plaintexts ([nvec][level+1][N] words): inverse
// NTT, the centred CRT and the division by the scale: [nvec][N] doubles.
func (r *Ring) DecodeCoeffs(flat []uint64, nvec, level int, scale float64) []float64 {
	d := r.upload(flat)
	defer r.free(d)
	out := make([]float64, nvec*r.N)
	r.check(C.sfg_ring_decode_coeffs(r.p, d, C.size_t((level+1)*r.N), C.int(nvec), C.int(level), C.double(scale), (*C.double)(unsafe.Pointer(&out[0]))), "ring_decode_coeffs")
	return out
}

// DecodeFloatVector: crypto.DecodeFloatVector (crypto.go:525-536) - the real parts of every slot of nvec NTT-domain plaintexts ([nvec][level+1][N] words, PCKSFinish's).
func (r *Ring) DecodeFloatVector(flat []uint64, nvec, level int, scale float64) []float64 {
	d := r.upload(flat)
	defer r.free(d)
	out := make([]float64, nvec*r.N/2)
	r.check(C.sfg_ring_decode_vectors(r.p, d, C.size_t((level+1)*r.N), C.int(nvec), C.int(level), C.double(scale), (*C.double)(unsafe.Pointer(&out[0])), nil), "ring_decode_vectors")
	return out
}

// DecryptFloatVector: crypto.DecryptFloatVector (crypto.go:489-510) under the loaded (whole) secret key: the real parts of every slot of nct ciphertexts.
func (r *Ring) DecryptFloatVector(flat []uint64, nct, level int, scale float64) []float64 {
	d := r.upload(flat)
	defer r.free(d)
	out := make([]float64, nct*r.N/2)
	r.check(C.sfg_ring_decrypt_vectors(r.p, d, C.int(nct), C.int(level), C.double(scale), (*C.double)(unsafe.Pointer(&out[0])), nil), "ring_decrypt_vectors")
	return out
}

// ---- the ring's collective key generation, local halves (mpc/mhe.go:24-105, 381-502; gring_keygen.hip): the twins of Ctx's methods of the same names, at the
// presets the specialised context does not serve.  PARITY UNPINNED against lattigo's dckks / drlwe protocols.  Shares come back as host words for
// mpc/aggregate.go; the aggregated words go back in and are installed from device memory.  SeedEncryptor first; the common reference polynomials come from the
// seed every party shares, through the one map of INTEGRATION.md.

// RingBuf is device memory of a ring that the caller frees.
type RingBuf struct {
	r     *Ring
	p     *C.uint64_t
	Words int
}

func (b *RingBuf) Free() {
	if b.p != nil {
		b.r.free(b.p)
		b.p = nil
	}
}

// LoadSecretKeyQP gives the ring skShard.Value over Q and P (mhe.go:31-46, NTT + Montgomery form); it also serves as LoadSecretKey.
func (r *Ring) LoadSecretKeyQP(sk *ckks.SecretKey) {
	nmod := r.NQ + r.NP
	flat := make([]uint64, nmod*r.N)
	for m := 0; m < nmod; m++ {
		copy(flat[m*r.N:(m+1)*r.N], sk.Value.Coeffs[m])
	}
	r.check(C.sfg_ring_load_secret_key_qp(r.p, (*C.uint64_t)(unsafe.Pointer(&flat[0])), 1), "ring_load_secret_key_qp")
}

func (r *Ring) keyBeta() int { return (r.NQ + r.NP - 1) / r.NP }

// CommonReferencePolys: crpGen.ReadNew() (mhe.go:49-59) for npoly consecutive polynomials over Q and P, starting at polynomial firstPoly of the stream under seed32.
func (r *Ring) CommonReferencePolys(seed32 []byte, firstPoly uint64, npoly int) *RingBuf {
	nmod := r.NQ + r.NP
	mod := make([]int32, npoly*nmod)
	for i := range mod {
		mod[i] = int32(i % nmod)
	}
	d := &RingBuf{r: r, p: r.alloc(npoly * nmod * r.N), Words: npoly * nmod * r.N}
	r.check(C.sfg_ring_crp_fill_dev(r.p, (*C.uint8_t)(unsafe.Pointer(&seed32[0])), C.uint64_t(firstPoly*uint64(nmod)), C.size_t(len(mod)), (*C.int)(unsafe.Pointer(&mod[0])), d.p), "ring_crp_fill")
	return d
}

// CollectivePubKeyGenShare: ckgProtocol.GenShare(sk, crp, pkShare) (mhe.go:91).
func (r *Ring) CollectivePubKeyGenShare(crp *RingBuf) []uint64 {
	words := (r.NQ + r.NP) * r.N
	d := r.alloc(words)
	defer r.free(d)
	r.check(C.sfg_ring_ckg_gen_share_sampled_dev(r.p, crp.p, d, nil), "ring_ckg_gen_share")
	return r.download(d, words)
}

// CollectivePubKeyGenFinish: ckgProtocol.GenPublicKey(pkAgg, crp, pk) (mhe.go:103); the key stays on the device.
func (r *Ring) CollectivePubKeyGenFinish(agg []uint64, crp *RingBuf) {
	d := r.upload(agg)
	defer r.free(d)
	r.check(C.sfg_ring_install_public_key_dev(r.p, d, crp.p), "ring_install_public_key")
}

// CollectiveRotKeyGenShares: rtgProtocol.GenShare for a batch of Galois elements (mhe.go:457-465); crp and the result are [len(gElems)][beta][nq+np][N].
func (r *Ring) CollectiveRotKeyGenShares(gElems []uint64, crp *RingBuf) []uint64 {
	d := r.alloc(crp.Words)
	defer r.free(d)
	r.check(C.sfg_ring_rtg_gen_shares_sampled_dev(r.p, (*C.uint64_t)(unsafe.Pointer(&gElems[0])), C.int(len(gElems)), crp.p, d, nil), "ring_rtg_gen_shares")
	return r.download(d, crp.Words)
}

// CollectiveRotKeyGenFinish: rtgProtocol.GenRotationKey for the batch (mhe.go:469).
func (r *Ring) CollectiveRotKeyGenFinish(gElems []uint64, agg []uint64, crp *RingBuf) {
	d := r.upload(agg)
	defer r.free(d)
	r.check(C.sfg_ring_install_rotkeys_dev(r.p, (*C.uint64_t)(unsafe.Pointer(&gElems[0])), C.int(len(gElems)), d, crp.p), "ring_install_rotkeys")
}

// CollectiveRelinKeyGenRound1: prot.GenShareRoundOne (mhe.go:492); uIndex names the ephemeral secret for round 2 (it is never stored).
func (r *Ring) CollectiveRelinKeyGenRound1(crp *RingBuf) (h0, h1 []uint64, uIndex uint64) {
	d0, d1 := r.alloc(crp.Words), r.alloc(crp.Words)
	defer r.free(d0)
	defer r.free(d1)
	var ui C.uint64_t
	r.check(C.sfg_ring_rkg_round1_sampled_dev(r.p, crp.p, d0, d1, nil, &ui), "ring_rkg_round1")
	return r.download(d0, crp.Words), r.download(d1, crp.Words), uint64(ui)
}

// CollectiveRelinKeyGenRound2: prot.GenShareRoundTwo on the aggregated round-one shares (mhe.go:495).
func (r *Ring) CollectiveRelinKeyGenRound2(h0agg, h1agg []uint64, uIndex uint64) []uint64 {
	a, b := r.upload(h0agg), r.upload(h1agg)
	defer r.free(a)
	defer r.free(b)
	d := r.alloc(len(h0agg))
	defer r.free(d)
	r.check(C.sfg_ring_rkg_round2_sampled_dev(r.p, a, b, C.uint64_t(uIndex), d, nil), "ring_rkg_round2")
	return r.download(d, len(h0agg))
}

// CollectiveRelinKeyGenFinish: prot.GenRelinearizationKey(outRound1, outRound2, evk) (mhe.go:498).
func (r *Ring) CollectiveRelinKeyGenFinish(round2agg, h1agg []uint64) {
	a, b := r.upload(round2agg), r.upload(h1agg)
	defer r.free(a)
	defer r.free(b)
	r.check(C.sfg_ring_install_relinkey_dev(r.p, a, b), "ring_install_relinkey")
}

// ExportRotKey: the stored key of a Galois element as [beta][2][nq+np][N] words, exactly (agg, crp); galEl 1 is the relinearisation key (mhe.go:60-81).
func (r *Ring) ExportRotKey(galEl uint64) []uint64 {
	out := make([]uint64, r.keyBeta()*2*(r.NQ+r.NP)*r.N)
	r.check(C.sfg_ring_export_rotkey(r.p, C.uint64_t(galEl), (*C.uint64_t)(unsafe.Pointer(&out[0]))), "ring_export_rotkey")
	return out
}

// ----------------------------------------------------------------------------------------------------------------
// The general ring's matrix products (gwas/matmult.go:1238-1505 at the presets other than PN14QP438).  The int8 matrix goes to device memory of the ring as it is
// (row-major, -1 = missing); aFlat is [s][nbr][2][inLevel+1][N] as Ctx.MatmulStream takes it.  The plaintext scale is the parameters' default scale.
func (r *Ring) mmFlags(square, transpose bool) C.uint {
	var f C.uint
	if square {
		f |= C.SFG_SQUARE
	}
	if transpose {
		f |= C.SFG_TRANSPOSE
	}
	return f
}

func (r *Ring) uploadGeno(geno []int8) unsafe.Pointer {
	d := r.allocBytes(len(geno))
	r.check(C.sfg_ring_memcpy_h2d(r.p, d, unsafe.Pointer(&geno[0]), C.size_t(len(geno))), "ring_memcpy_h2d")
	return d
}

// MatMult - MatMult4Stream (matmult.go:1238-1505): out [s][mct][2][maxLevel][N] at level maxLevel-1, the deterministic sum (the caller adds the fresh zeros).
func (r *Ring) MatMult(aFlat []uint64, s, inLevel, maxLevel int, geno []int8, nrow, ncol int, square, transpose bool) []uint64 {
	slots := r.N / 2
	cols := ncol
	if transpose {
		cols = nrow
	}
	mct := (cols-1)/slots + 1
	dG := r.uploadGeno(geno)
	defer r.freeBytes(dG)
	return r.unary(aFlat, s*mct*2*maxLevel*r.N, "ring_matmul", func(dA, dOut *C.uint64_t) C.int {
		return C.sfg_ring_matmul_dev(r.p, dA, C.int(s), C.int(inLevel), C.int(maxLevel), (*C.int8_t)(dG), C.size_t(nrow), C.size_t(ncol), C.size_t(ncol),
			r.mmFlags(square, transpose), C.double(r.Params.Scale()), dOut)
	})
}

// EncoderResolved is the number of diagonal coefficients the products re-derived exactly (inside the encoder's band of a rounding tie) since the last reset.
func (r *Ring) EncoderResolved(reset bool) uint64 {
	var n C.ulonglong
	flag := 0
	if reset {
		flag = 1
	}
	r.check(C.sfg_ring_encoder_resolved(r.p, &n, C.int(flag)), "ring_encoder_resolved")
	return uint64(n)
}

// MatMultD is ceil(sqrt(slots)): the number of baby and of giant steps (matmult.go:1249).
func (r *Ring) MatMultD() int {
	d := 1
	for d*d < r.N/2 {
		d++
	}
	return d
}

// MatMultAccumulate - matmult.go:1280-1439 and the reduction of :343-366 for operand block rows [b0, b1): acc [mct][d][s][2][maxLevel][N] canonical residues and
// the giants that became active.  Partial accumulators of disjoint ranges add up modulo q (Binary "add" on their words) to the whole's.
func (r *Ring) MatMultAccumulate(aFlat []uint64, s, inLevel, maxLevel int, geno []int8, nrow, ncol int, square, transpose bool, b0, b1 int) ([]uint64, []uint8) {
	slots, d := r.N/2, r.MatMultD()
	cols := ncol
	if transpose {
		cols = nrow
	}
	mct := (cols-1)/slots + 1
	active := make([]uint8, d)
	dG := r.uploadGeno(geno)
	defer r.freeBytes(dG)
	acc := r.unary(aFlat, mct*d*s*2*maxLevel*r.N, "ring_matmul_accumulate", func(dA, dOut *C.uint64_t) C.int {
		return C.sfg_ring_matmul_accumulate_dev(r.p, dA, C.int(s), C.int(inLevel), C.int(maxLevel), (*C.int8_t)(dG), C.size_t(nrow), C.size_t(ncol), C.size_t(ncol),
			r.mmFlags(square, transpose), C.double(r.Params.Scale()), C.int(b0), C.int(b1), dOut, (*C.uint8_t)(unsafe.Pointer(&active[0])))
	})
	return acc, active
}

// MatMultFinalize - matmult.go:1443-1502: the active giants g > 0 rotated by -g d at level maxLevel-1 and summed: out [s][mct][2][maxLevel][N].
func (r *Ring) MatMultFinalize(acc []uint64, active []uint8, s, maxLevel, mct int) []uint64 {
	return r.unary(acc, s*mct*2*maxLevel*r.N, "ring_matmul_finalize", func(dAcc, dOut *C.uint64_t) C.int {
		return C.sfg_ring_matmul_finalize_dev(r.p, dAcc, (*C.uint8_t)(unsafe.Pointer(&active[0])), C.int(s), C.int(maxLevel), C.int(mct), 0, C.int(r.MatMultD()), 0, dOut)
	})
}

// FlattenCipherMatrix: rows [s][nbr] of ciphertexts -> [s][nbr][2][level+1][N], Ctx's own layout on the ring's parameters.
func (r *Ring) FlattenCipherMatrix(rows [][]*ckks.Ciphertext, level int) []uint64 {
	return r.host().FlattenCipherMatrix(rows, level)
}

// CanEncrypt: a public key is loaded and the sampler is keyed (Ring.LoadPublicKey, Ring.SeedEncryptor): the fresh zeros of a product can be made on the device.
func (r *Ring) CanEncrypt() bool { return r.HasPublicKey() }
