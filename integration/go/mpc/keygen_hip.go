// keygen_hip.go - the local halves of CollectiveInit (mpc/mhe.go:24-105, 381-502) on the device, at every CKKS preset: the specialised context at PN14QP438
// (hip.Default), the general ring at the others (hip.DefaultRing, made by hip.InitRing before any key exists: pass nil key sets).  The aggregation between the
// halves stays where it is (mpc/aggregate.go:121-240): each function returns the party's share as host words and takes the aggregated words back.
// PARITY UNPINNED (INTEGRATION.md, "Generating the keys on the device"): every party, a CPU-only one included, expands the common reference polynomials from the
// shared 32-byte seed through the one map stated there.
package mpc

import (
	"github.com/hhcho/sfgwas/hip"
	"github.com/ldsec/lattigo/v2/ckks"
)

// onRing says whether the process runs a preset the general ring serves.
func onRing(params *ckks.Parameters) *hip.Ring {
	if r := hip.DefaultRing; r != nil && r.Params == params {
		return r
	}
	return nil
}

// HipLoadSecretKeyQP: skShard over Q and P (mhe.go:31-46), then the sampler key.
func HipLoadSecretKeyQP(params *ckks.Parameters, sk *ckks.SecretKey) {
	if r := onRing(params); r != nil {
		r.LoadSecretKeyQP(sk)
		r.SeedEncryptor()
		return
	}
	h := hip.Default
	h.LoadSecretKeyQP(sk)
	h.SeedEncryptor()
}

// HipCollectivePubKeyGen: mhe.go:83-105 around `aggregate` (AggregatePubKeyShares on flat words).
func HipCollectivePubKeyGen(params *ckks.Parameters, seed32 []byte, aggregate func(share []uint64) []uint64) {
	if r := onRing(params); r != nil {
		crp := r.CommonReferencePolys(seed32, 0, 1)
		defer crp.Free()
		r.CollectivePubKeyGenFinish(aggregate(r.CollectivePubKeyGenShare(crp)), crp)
		return
	}
	h := hip.Default
	crp := h.CommonReferencePolys(seed32, 0, 1)
	defer crp.Free()
	h.CollectivePubKeyGenFinish(aggregate(h.CollectivePubKeyGenShare(crp)), crp)
}

// HipCollectiveRelinKeyGen: mhe.go:478-502; the common reference polynomials are polynomials 1 .. beta of the stream.
func HipCollectiveRelinKeyGen(params *ckks.Parameters, seed32 []byte, beta int, aggregate func(share []uint64) []uint64) {
	if r := onRing(params); r != nil {
		crp := r.CommonReferencePolys(seed32, 1, beta)
		defer crp.Free()
		h0, h1, uIndex := r.CollectiveRelinKeyGenRound1(crp)
		h0agg, h1agg := aggregate(h0), aggregate(h1)
		r.CollectiveRelinKeyGenFinish(aggregate(r.CollectiveRelinKeyGenRound2(h0agg, h1agg, uIndex)), h1agg)
		return
	}
	h := hip.Default
	crp := h.CommonReferencePolys(seed32, 1, beta)
	defer crp.Free()
	h0, h1, uIndex := h.CollectiveRelinKeyGenRound1(crp)
	h0agg, h1agg := aggregate(h0), aggregate(h1)
	h.CollectiveRelinKeyGenFinish(aggregate(h.CollectiveRelinKeyGenRound2(h0agg, h1agg, uIndex)), h1agg)
}

// HipCollectiveRotKeyGen: mhe.go:381-476 for the sorted Galois elements, in batches of `batch` keys (the caller's memory knob; the ring runs any batch in
// chunks of at most 1024 keys); batch k's common reference polynomials start at polynomial 1 + beta (1 + k batch) of the stream.
func HipCollectiveRotKeyGen(params *ckks.Parameters, seed32 []byte, beta int, gElems []uint64, batch int, aggregate func(share []uint64) []uint64) {
	for k0 := 0; k0 < len(gElems); k0 += batch {
		k1 := k0 + batch
		if k1 > len(gElems) {
			k1 = len(gElems)
		}
		first := uint64(1 + beta*(1+k0))
		if r := onRing(params); r != nil {
			crp := r.CommonReferencePolys(seed32, first, (k1-k0)*beta)
			r.CollectiveRotKeyGenFinish(gElems[k0:k1], aggregate(r.CollectiveRotKeyGenShares(gElems[k0:k1], crp)), crp)
			crp.Free()
			continue
		}
		h := hip.Default
		crp := h.CommonReferencePolys(seed32, first, (k1-k0)*beta)
		h.CollectiveRotKeyGenFinish(gElems[k0:k1], aggregate(h.CollectiveRotKeyGenShares(gElems[k0:k1], crp)), crp)
		crp.Free()
	}
}
