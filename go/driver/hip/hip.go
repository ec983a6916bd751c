/*
Package hip is the MI355X backend for the hot path of github.com/IBM/mathlib: it plugs in beside
driver/amcl, driver/gurvy and driver/kilic behind the unchanged driver.Curve interface
(driver/math.go:49-180) and overrides ONLY the data-parallel methods -- MultiScalarMul, Pairing,
Pairing2, FExp -- with calls into libmlhip.so (C ABI: include/mlhip.h).  Everything else (the ~40
remaining Curve methods, element arithmetic, serialization, hashing) is inherited bit-for-bit from the
gurvy BLS12-381 driver by embedding, the way BBSCurve overrides four methods of Curve in
driver/gurvy/bls12381/bls12-381.go:785-867.

Memory is handed over with zero conversion: gnark-crypto's G1Affine / G2Affine / fr.Element / GT are
plain arrays of little-endian uint64 limbs in Montgomery form, which is exactly the layout the kernels
use (driver/gurvy/custom.go:24-40 proves the layout for fp.Element; init() below re-checks the sizes).

NOTE: this file has never been compiled -- the build image has no Go toolchain (SURVEY.md, headline
fact 3).  It is the binding a maintainer would add; INTEGRATION.md walks through it.  The same ABI is
exercised by the Python mirror mathlib_amd/driver.py, which the test-suite runs on the GPU.

Failure convention: like every reference driver this package panics on failure (there are no error
returns in package driver; cf. driver/gurvy/bn254.go:249-251).  There is no CPU fallback: without a
usable GPU the hot methods panic with the library's message; the inherited methods keep working, so
registering the curve in math.Curves never needs a GPU (GenGt at package init uses the embedded
driver: driver/gurvy/bls12381/bls12-381.go:490-497).
*/
package hip

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../mathlib_amd -lmlhip -Wl,-rpath,${SRCDIR}/../../../mathlib_amd
#include <stdlib.h>
#include "mlhip.h"
#include "mlhip_bits.h"
#include "mlhip_products.h"
#include "mlhip_subgroup.h"
#include "mlhip_bases_set.h"
#include "mlhip_sum_batch.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"unsafe"

	"github.com/IBM/mathlib/driver"
	gurvy381 "github.com/IBM/mathlib/driver/gurvy/bls12381"
	bls12381 "github.com/consensys/gnark-crypto/ecc/bls12-381"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
)

// WindowC is the Pippenger window (0 = chosen from n; BASELINE config 2 uses 16).
var WindowC = 0

// The GPU is a throughput device.  Measured on one MI355X through this ABI (tools/perf_latency.py,
// profiles/r03_perf_latency.txt): a MultiScalarMul of 2 points takes 0.3-0.4 ms, of 2^20 points 4.2 ms; but ONE Miller
// loop takes 2.5 ms and ONE final exponentiation 5.2 ms, because a single pairing occupies a single quad of lanes
// (65 536 pairings take 17.7 ms).  gnark on the CPU does a single pairing in about a millisecond.  Hence:
//
// MinDeviceMSM: MultiScalarMul with fewer pairs stays on the embedded gurvy driver.  A host-slice MSM costs the device
// a flat 0.39-0.51 ms up to 2^10 pairs and 0.55-0.9 ms from 2^12 to 2^16 (profiles/r03_min_device_msm.txt,
// profiles/r03_perf_small_msm.txt).  The CPU side cannot be measured with gnark (no Go toolchain here or on the GPU
// box: profiles/r03_go_probe.txt); the stated stand-in, the C restatement (oracle/cref, tools/perf_min_device_msm.py)
// timed on the GPU box's own cores, needs on ONE thread 0.40 ms for 2 pairs, 2.6 ms for 32 and 29 ms for 2^10, on 8
// threads 0.52 / 0.78 / 4.4 ms, and never gets under 2 ms on all 64 -- the device is level with it from the second
// pair.  gnark with ADX assembly is several times faster than that plain-C port, which puts the break-even near 8-32
// pairs; 32 keeps the tiny proofs-of-knowledge MSMs (perf_test.go:198-224, 3-7 pairs) on the CPU.
var MinDeviceMSM = 32

// MinDeviceMSMBatch: MultiScalarMulBatch / Mul2Batch with fewer pairs in all stay on the embedded gurvy driver;
// MaxBatchSegment: a segment of this many pairs or more is sent to MultiScalarMul on its own.  MinDeviceMSMBatch was
// measured with tools/perf_msm_batch.py (profiles/msm_batch_grid.jsonl, DESIGN.md section 8): a batch call costs the
// device 3-7 ms while it is not filled, and the C restatement on the GPU box's 16 cores needs 12-47 ms for 2 048 pairs; as
// for MinDeviceMSM, gnark itself cannot be timed here, and its ADX code being several times faster than that port puts the
// break-even near 2^11 pairs.  MaxBatchSegment follows tools/perf_msm_batch_bucket.py (profiles/msm_batch_bucket_ab.txt):
// the library sends segments of 512 pairs or more through its bucket route, and with it one batch call of 2^14-pair
// segments is level with or ahead of as many single mlhip_msm_g1 calls (BLS12-381: 11.8 against 12.1 ms for 16 of them,
// 25 against 47 ms for 64); from 2^16 pairs per segment on the single calls are ahead in every measured cell.
var MinDeviceMSMBatch = 2048
var MaxBatchSegment = 65536

// MinDevicePairingBatch: PairingBatch with fewer pairs stays on the embedded gurvy driver.  Any batch up to 16 384
// pairs costs one wave time on the device (5.2 ms on an MI355X, one pairing per quad of lanes:
// profiles/r02_perf_pairing_quads.txt); a CPU
// core needs about a millisecond per pairing, so a few hundred pairs are where the device starts to win.
var MinDevicePairingBatch = 256

// DevicePairing: when false (default) the single-shot Pairing / Pairing2 / FExp stay on the embedded gurvy driver
// and only the batched entry points (PairingBatch) use the GPU.  Mixing is safe: FExp of either Miller loop's
// output is the same canonical Gt (SURVEY.md section 8c).
var DevicePairing = false

func init() {
	// the C ABI assumes gnark's in-memory layout; refuse to run if it ever changes
	if unsafe.Sizeof(bls12381.G1Affine{}) != 96 || unsafe.Sizeof(bls12381.G2Affine{}) != 192 ||
		unsafe.Sizeof(bls12381.GT{}) != 576 || unsafe.Sizeof(fr.Element{}) != 32 {
		panic("hip: gnark-crypto element layout changed; libmlhip.so expects 96/192/576/32-byte elements")
	}
}

// check runs one library call and panics with the library's message when it fails.  libmlhip keeps the message (and
// a thread's optional device pin) per OS thread, and goroutines migrate between threads from one cgo call to the
// next: the goroutine is locked to its thread from the call until the message has been read.  Device selection does
// not rely on thread state at all -- it is the process-wide list of SetDevices below.
func check(call func() C.int) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := call(); rc != 0 {
		panic(fmt.Sprintf("hip: libmlhip error %d: %s", int(rc), C.GoString(C.mlhip_last_error())))
	}
}

// SetDevices sets the GPUs of this process (mlhip_init; no argument = every visible device; the environment variable
// MLHIP_DEVICES does the same).  With two or more, MultiScalarMul / MultiScalarMulG2 / NewBases of 2^21 pairs and more
// and PairingBatch of 2^17 pairs and more are cut into contiguous shards, one per GPU, each run by its own host thread
// inside the library; the per-GPU partial sums are added on the host (SURVEY.md 8e; BASELINE configs 4 and 5).
// Smaller calls run on the first listed device.
func SetDevices(devices ...int) {
	var p *C.int
	d := make([]C.int, len(devices))
	for i, v := range devices {
		d[i] = C.int(v)
	}
	if len(d) > 0 {
		p = &d[0]
	}
	check(func() C.int { return C.mlhip_init(p, C.int(len(d))) })
}

// Curve is the gurvy BLS12-381 curve with its hot methods moved to the GPU.
type Curve struct {
	gurvy381.Curve
}

func NewCurve() *Curve { return &Curve{*gurvy381.NewCurve()} }

// MultiScalarMul replaces driver/gurvy/bls12381/bls12-381.go:766-783 (gather + G1Jac.MultiExp +
// FromJacobian).  The gather into contiguous arrays stays (the interface hands over boxed elements);
// scalars are passed as fr.Element in Montgomery form, exactly what the gurvy driver feeds MultiExp.
func (c *Curve) MultiScalarMul(a []driver.G1, b []driver.Zr) driver.G1 {
	n := len(a)
	points := make([]bls12381.G1Affine, n)
	scalars := make([]fr.Element, len(b))
	for i := range a {
		points[i] = a[i].(*gurvy381.G1).G1Affine
		scalars[i] = gurvy381.ZrValue(b[i]) // accessor for Zr.val (bls12-381.go:49-52); see INTEGRATION.md
	}
	out := &gurvy381.G1{}
	if len(b) != n || n == 0 {
		// gnark's MultiExp errors on a length mismatch and the driver drops the error: identity
		return out
	}
	if n < MinDeviceMSM {
		return c.Curve.MultiScalarMul(a, b)
	}
	check(func() C.int {
		return C.mlhip_msm_g1(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), C.int(WindowC),
		unsafe.Pointer(&out.G1Affine))
	})
	return out
}

// MultiScalarMulBatch returns MultiScalarMul(a[i], b[i]) for every i -- an idemix / BBS verifier's many small MSMs --
// with one device call (mlhip_msm_batch: chunks of a few pairs per lane, buckets for long segments, DESIGN.md section 8).  Every segment keeps
// MultiScalarMul's rules: fewer scalars than points panics (index out of range, math.go:960-969), more gives the
// identity.  A batch of fewer than MinDeviceMSMBatch pairs in all stays on the embedded gurvy driver, and a segment of
// MaxBatchSegment pairs or more goes to MultiScalarMul on its own (mlhip_msm_g1 is faster there).
func (c *Curve) MultiScalarMulBatch(a [][]driver.G1, b [][]driver.Zr) []driver.G1 {
	return c.msmBatchG1(a, b, false)
}

// MultiScalarMulBatchSubgroup is MultiScalarMulBatch for points the caller knows to be in G1 (decoded with the subgroup
// check, issuer keys, generators, outputs of earlier MSMs): the same results with half of the chunks' doublings, from the
// curve's endomorphism and a split of every scalar (mlhip_msm_batch_subgroup, DESIGN.md section 19).  A point outside G1
// gives an undefined result for its own segment; MultiScalarMulBatch accepts any point of the curve.  On BN254 every point
// of the curve is in G1 (the lattice split of DESIGN.md section 20 runs): only a point off the curve breaks the promise.
func (c *Curve) MultiScalarMulBatchSubgroup(a [][]driver.G1, b [][]driver.Zr) []driver.G1 {
	return c.msmBatchG1(a, b, true)
}

func (c *Curve) msmBatchG1(a [][]driver.G1, b [][]driver.Zr, subgroup bool) []driver.G1 {
	if len(a) != len(b) {
		panic("hip: MultiScalarMulBatch length mismatch")
	}
	k := len(a)
	out := make([]driver.G1, k)
	total := 0
	for i := range a {
		if len(b[i]) < len(a[i]) {
			_ = b[i][len(a[i])-1] // the reference's index out of range
		}
		if len(b[i]) == len(a[i]) && len(a[i]) < MaxBatchSegment {
			total += len(a[i])
		}
	}
	if total < MinDeviceMSMBatch {
		for i := range a {
			out[i] = c.MultiScalarMul(a[i], b[i])
		}
		return out
	}
	offsets := make([]uint64, k+1)
	points := make([]bls12381.G1Affine, 0, total)
	scalars := make([]fr.Element, 0, total)
	for i := range a {
		offsets[i+1] = offsets[i]
		if len(b[i]) != len(a[i]) || len(a[i]) >= MaxBatchSegment {
			continue // the identity, or (below) a segment of its own
		}
		for j := range a[i] {
			points = append(points, a[i][j].(*gurvy381.G1).G1Affine)
			scalars = append(scalars, gurvy381.ZrValue(b[i][j]))
		}
		offsets[i+1] += uint64(len(a[i]))
	}
	res := make([]bls12381.G1Affine, k)
	check(func() C.int {
		if subgroup {
			return C.mlhip_msm_batch_subgroup(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1, unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1,
				(*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.size_t(k), unsafe.Pointer(&res[0]))
		}
		return C.mlhip_msm_batch(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1, unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1,
			(*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.size_t(k), unsafe.Pointer(&res[0]))
	})
	for i := range res {
		if len(b[i]) == len(a[i]) && len(a[i]) >= MaxBatchSegment {
			out[i] = c.MultiScalarMul(a[i], b[i])
		} else {
			out[i] = &gurvy381.G1{G1Affine: res[i]}
		}
	}
	return out
}

// MultiScalarMulG2BatchSubgroup returns MultiScalarMulG2(a[i], b[i]) for every i, for points the caller knows to be in G2,
// with one device call (mlhip_msm_batch_subgroup: a quarter of the chunks' doublings).  The length rules are
// MultiScalarMulBatch's; a batch of fewer than MinDeviceMSMBatch pairs in all, and a segment of MaxBatchSegment pairs or more,
// go to MultiScalarMulG2.
func (c *Curve) MultiScalarMulG2BatchSubgroup(a [][]driver.G2, b [][]driver.Zr) []driver.G2 {
	if len(a) != len(b) {
		panic("hip: MultiScalarMulG2BatchSubgroup length mismatch")
	}
	k := len(a)
	out := make([]driver.G2, k)
	total := 0
	for i := range a {
		if len(b[i]) < len(a[i]) {
			_ = b[i][len(a[i])-1] // the reference's index out of range
		}
		if len(b[i]) == len(a[i]) && len(a[i]) < MaxBatchSegment {
			total += len(a[i])
		}
	}
	if total < MinDeviceMSMBatch {
		for i := range a {
			out[i] = c.MultiScalarMulG2(a[i], b[i])
		}
		return out
	}
	offsets := make([]uint64, k+1)
	points := make([]bls12381.G2Affine, 0, total)
	scalars := make([]fr.Element, 0, total)
	for i := range a {
		offsets[i+1] = offsets[i]
		if len(b[i]) != len(a[i]) || len(a[i]) >= MaxBatchSegment {
			continue // the identity, or (below) a segment of its own
		}
		for j := range a[i] {
			points = append(points, a[i][j].(*gurvy381.G2).G2Affine)
			scalars = append(scalars, gurvy381.ZrValue(b[i][j]))
		}
		offsets[i+1] += uint64(len(a[i]))
	}
	res := make([]bls12381.G2Affine, k)
	check(func() C.int {
		return C.mlhip_msm_batch_subgroup(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2, unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1,
			(*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.size_t(k), unsafe.Pointer(&res[0]))
	})
	for i := range res {
		if len(b[i]) == len(a[i]) && len(a[i]) >= MaxBatchSegment {
			out[i] = c.MultiScalarMulG2(a[i], b[i])
		} else {
			out[i] = &gurvy381.G2{G2Affine: res[i]}
		}
	}
	return out
}

// Mul2Batch returns g[i].Mul2(e[i], q[i], f[i]) for every i: MultiScalarMulBatch over segments of two pairs.
func (c *Curve) Mul2Batch(g []driver.G1, e []driver.Zr, q []driver.G1, f []driver.Zr) []driver.G1 {
	n := len(g)
	if len(e) != n || len(q) != n || len(f) != n {
		panic("hip: Mul2Batch length mismatch")
	}
	a := make([][]driver.G1, n)
	b := make([][]driver.Zr, n)
	for i := range g {
		a[i] = []driver.G1{g[i], q[i]}
		b[i] = []driver.Zr{e[i], f[i]}
	}
	return c.MultiScalarMulBatch(a, b)
}

// Pairing replaces bls12-381.go:448-455: Miller loop only, compare after FExp.
func (c *Curve) Pairing(p2 driver.G2, p1 driver.G1) driver.Gt {
	if !DevicePairing {
		return c.Curve.Pairing(p2, p1)
	}
	out := &gurvy381.Gt{}
	check(func() C.int {
		return C.mlhip_miller_loop(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&p1.(*gurvy381.G1).G1Affine), unsafe.Pointer(&p2.(*gurvy381.G2).G2Affine),
		1, 1, unsafe.Pointer(&out.GT))
	})
	return out
}

// Pairing2 replaces bls12-381.go:457-464 (one shared Miller loop over two pairs).
func (c *Curve) Pairing2(p2a, p2b driver.G2, p1a, p1b driver.G1) driver.Gt {
	if !DevicePairing {
		return c.Curve.Pairing2(p2a, p2b, p1a, p1b)
	}
	g1 := [2]bls12381.G1Affine{p1a.(*gurvy381.G1).G1Affine, p1b.(*gurvy381.G1).G1Affine}
	g2 := [2]bls12381.G2Affine{p2a.(*gurvy381.G2).G2Affine, p2b.(*gurvy381.G2).G2Affine}
	out := &gurvy381.Gt{}
	check(func() C.int {
		return C.mlhip_miller_loop(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&g1[0]), unsafe.Pointer(&g2[0]), 2, 1, unsafe.Pointer(&out.GT))
	})
	return out
}

// FExp replaces bls12-381.go:466-468.
func (c *Curve) FExp(a driver.Gt) driver.Gt {
	if !DevicePairing {
		return c.Curve.FExp(a)
	}
	out := &gurvy381.Gt{}
	check(func() C.int {
		return C.mlhip_final_exp(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&a.(*gurvy381.Gt).GT), 1, unsafe.Pointer(&out.GT))
	})
	return out
}

// ---- additive API (not in driver.Curve; needed by BASELINE configs 3 and 4) --------------------

// MultiScalarMulG2 = sum of G2.Mul + Add (bls12-381.go:342-358) as one MSM.
func (c *Curve) MultiScalarMulG2(a []driver.G2, b []driver.Zr) driver.G2 {
	n := len(a)
	points := make([]bls12381.G2Affine, n)
	scalars := make([]fr.Element, len(b))
	for i := range a {
		points[i] = a[i].(*gurvy381.G2).G2Affine
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	out := &gurvy381.G2{}
	if len(b) != n || n == 0 {
		return out
	}
	check(func() C.int {
		return C.mlhip_msm_g2(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), C.int(WindowC),
		unsafe.Pointer(&out.G2Affine))
	})
	return out
}

// MultiScalarMulShort = MultiScalarMul for scalars known to be below 2^bits (a batch verifier's 64- or 128-bit
// randomisers): sum of [b[i] mod 2^bits] a[i] through mlhip_msm_bits, the same point as MultiScalarMul when the scalars
// keep the promise, in fewer windows.  bits = 0 means full width.  Same length rules as MultiScalarMul.
func (c *Curve) MultiScalarMulShort(a []driver.G1, b []driver.Zr, bits int) driver.G1 {
	n := len(a)
	if len(b) < n {
		_ = b[n-1] // the reference's index out of range (math.go:960-969)
	}
	out := &gurvy381.G1{}
	if len(b) != n || n == 0 {
		return out
	}
	points := make([]bls12381.G1Affine, n)
	scalars := make([]fr.Element, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G1).G1Affine
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	check(func() C.int {
		return C.mlhip_msm_bits(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1,
			unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1, C.int(bits), C.size_t(n), C.int(WindowC),
			unsafe.Pointer(&out.G1Affine))
	})
	return out
}

// MultiScalarMulG2Short is the same in G2.
func (c *Curve) MultiScalarMulG2Short(a []driver.G2, b []driver.Zr, bits int) driver.G2 {
	n := len(a)
	if len(b) < n {
		_ = b[n-1]
	}
	out := &gurvy381.G2{}
	if len(b) != n || n == 0 {
		return out
	}
	points := make([]bls12381.G2Affine, n)
	scalars := make([]fr.Element, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G2).G2Affine
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	check(func() C.int {
		return C.mlhip_msm_bits(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2,
			unsafe.Pointer(&points[0]), unsafe.Pointer(&scalars[0]), 1, C.int(bits), C.size_t(n), C.int(WindowC),
			unsafe.Pointer(&out.G2Affine))
	})
	return out
}

// SumG1 = a[0] + a[1] + ...: G1.Add in a loop (bls12-381.go, Add) as one call.  Short lists are added on the host by
// the library; long ones (aggregating signatures, folding proofs) are summed on the device (mlhip_g1_sum,
// MLHIP_SUM_DEVICE_MIN).  An empty list gives the identity.
func (c *Curve) SumG1(a []driver.G1) driver.G1 {
	out := &gurvy381.G1{}
	n := len(a)
	if n == 0 {
		return out
	}
	points := make([]bls12381.G1Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G1).G1Affine
	}
	check(func() C.int {
		return C.mlhip_g1_sum(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&points[0]), C.size_t(n), unsafe.Pointer(&out.G1Affine))
	})
	return out
}

// SumG2 is SumG1 in G2 (mlhip_g2_sum): aggregating public keys.
func (c *Curve) SumG2(a []driver.G2) driver.G2 {
	out := &gurvy381.G2{}
	n := len(a)
	if n == 0 {
		return out
	}
	points := make([]bls12381.G2Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G2).G2Affine
	}
	check(func() C.int {
		return C.mlhip_g2_sum(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&points[0]), C.size_t(n), unsafe.Pointer(&out.G2Affine))
	})
	return out
}

// SumG1Batch returns SumG1(a[i]) for every i -- K committees' keys, K aggregate signatures, K folded proofs -- with one
// device call (mlhip_sum_batch: strided slices of every list per lane, one mixed addition per point, DESIGN.md section 21).
// An empty list gives the identity.  There is no host fallback: without a device the call panics.
func (c *Curve) SumG1Batch(a [][]driver.G1) []driver.G1 {
	k := len(a)
	out := make([]driver.G1, k)
	if k == 0 {
		return out
	}
	offsets := make([]uint64, k+1)
	var points []bls12381.G1Affine
	for i := range a {
		for j := range a[i] {
			points = append(points, a[i][j].(*gurvy381.G1).G1Affine)
		}
		offsets[i+1] = offsets[i] + uint64(len(a[i]))
	}
	var pp unsafe.Pointer
	if len(points) > 0 {
		pp = unsafe.Pointer(&points[0])
	}
	res := make([]bls12381.G1Affine, k)
	check(func() C.int {
		return C.mlhip_sum_batch(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1, pp, (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
			C.size_t(k), unsafe.Pointer(&res[0]))
	})
	for i := range res {
		out[i] = &gurvy381.G1{G1Affine: res[i]}
	}
	return out
}

// SumG2Batch is SumG1Batch in G2.
func (c *Curve) SumG2Batch(a [][]driver.G2) []driver.G2 {
	k := len(a)
	out := make([]driver.G2, k)
	if k == 0 {
		return out
	}
	offsets := make([]uint64, k+1)
	var points []bls12381.G2Affine
	for i := range a {
		for j := range a[i] {
			points = append(points, a[i][j].(*gurvy381.G2).G2Affine)
		}
		offsets[i+1] = offsets[i] + uint64(len(a[i]))
	}
	var pp unsafe.Pointer
	if len(points) > 0 {
		pp = unsafe.Pointer(&points[0])
	}
	res := make([]bls12381.G2Affine, k)
	check(func() C.int {
		return C.mlhip_sum_batch(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2, pp, (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
			C.size_t(k), unsafe.Pointer(&res[0]))
	})
	for i := range res {
		out[i] = &gurvy381.G2{G2Affine: res[i]}
	}
	return out
}

// MultiScalarMulG1G2 = (MultiScalarMul(a1, b), MultiScalarMulG2(a2, b)) for ONE scalar vector (BASELINE configs[3]: a
// prover's G1 and G2 MSM over the same witness): the scalars travel and are sorted once, both groups accumulate from
// the same bucket lists.  Mismatched lengths give the identities, as MultiScalarMul does (bls12-381.go:777).
func (c *Curve) MultiScalarMulG1G2(a1 []driver.G1, a2 []driver.G2, b []driver.Zr) (driver.G1, driver.G2) {
	n := len(a1)
	o1, o2 := &gurvy381.G1{}, &gurvy381.G2{}
	if len(a2) != n || len(b) != n || n == 0 {
		return o1, o2
	}
	p1 := make([]bls12381.G1Affine, n)
	p2 := make([]bls12381.G2Affine, n)
	scalars := make([]fr.Element, n)
	for i := 0; i < n; i++ {
		p1[i] = a1[i].(*gurvy381.G1).G1Affine
		p2[i] = a2[i].(*gurvy381.G2).G2Affine
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	check(func() C.int {
		return C.mlhip_msm_g1g2(C.MLHIP_CURVE_BLS12_381,
			unsafe.Pointer(&p1[0]), unsafe.Pointer(&p2[0]), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), C.int(WindowC),
			unsafe.Pointer(&o1.G1Affine), unsafe.Pointer(&o2.G2Affine))
	})
	return o1, o2
}

// PairingBatch returns FExp(Pairing(g2s[i], g1s[i])) for every i with one kernel launch.
func (c *Curve) PairingBatch(g2s []driver.G2, g1s []driver.G1) []driver.Gt {
	n := len(g1s)
	if len(g2s) != n {
		panic("hip: PairingBatch length mismatch")
	}
	if n == 0 {
		return nil
	}
	if n < MinDevicePairingBatch {
		out := make([]driver.Gt, n)
		for i := range g1s {
			out[i] = c.Curve.FExp(c.Curve.Pairing(g2s[i], g1s[i]))
		}
		return out
	}
	p := make([]bls12381.G1Affine, n)
	q := make([]bls12381.G2Affine, n)
	for i := range g1s {
		p[i] = g1s[i].(*gurvy381.G1).G1Affine
		q[i] = g2s[i].(*gurvy381.G2).G2Affine
	}
	gts := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_pairing_batch(C.MLHIP_CURVE_BLS12_381,
		unsafe.Pointer(&p[0]), unsafe.Pointer(&q[0]), C.size_t(n), unsafe.Pointer(&gts[0]))
	})
	out := make([]driver.Gt, n)
	for i := range gts {
		out[i] = &gurvy381.Gt{GT: gts[i]}
	}
	return out
}

// MillerLoopProducts returns out[k] = prod_j Pairing(g2s[k][j], g1s[k][j]): K products of m pairs each, any m, in one device
// call (include/mlhip.h: "products of any length", mlhip_miller_loop_products); not final-exponentiated, like Pairing.  Every
// product has the same length: a shorter one is padded with pairs at infinity.
func (c *Curve) MillerLoopProducts(g2s [][]driver.G2, g1s [][]driver.G1) []driver.Gt {
	n := len(g1s)
	if len(g2s) != n {
		panic("hip: MillerLoopProducts length mismatch")
	}
	if n == 0 {
		return nil
	}
	m := len(g1s[0])
	if m == 0 {
		panic("hip: MillerLoopProducts needs at least one pair per product")
	}
	p := make([]bls12381.G1Affine, 0, n*m)
	q := make([]bls12381.G2Affine, 0, n*m)
	for k := range g1s {
		if len(g1s[k]) != m || len(g2s[k]) != m {
			panic("hip: MillerLoopProducts: every product takes the same number of G1 and of G2 points")
		}
		for j := 0; j < m; j++ {
			p = append(p, g1s[k][j].(*gurvy381.G1).G1Affine)
			q = append(q, g2s[k][j].(*gurvy381.G2).G2Affine)
		}
	}
	gts := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_miller_loop_products(C.MLHIP_CURVE_BLS12_381,
			unsafe.Pointer(&p[0]), unsafe.Pointer(&q[0]), C.size_t(m), C.size_t(n), unsafe.Pointer(&gts[0]))
	})
	out := make([]driver.Gt, n)
	for i := range gts {
		out[i] = &gurvy381.Gt{GT: gts[i]}
	}
	return out
}

// PairingProducts returns out[k] = FExp(prod_j Pairing(g2s[k][j], g1s[k][j])): FExp of MillerLoopProducts, through
// mlhip_final_exp.
func (c *Curve) PairingProducts(g2s [][]driver.G2, g1s [][]driver.G1) []driver.Gt {
	ml := c.MillerLoopProducts(g2s, g1s)
	n := len(ml)
	if n == 0 {
		return nil
	}
	in := make([]bls12381.GT, n)
	for i := range ml {
		in[i] = ml[i].(*gurvy381.Gt).GT
	}
	gts := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_final_exp(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), C.size_t(n), unsafe.Pointer(&gts[0]))
	})
	out := make([]driver.Gt, n)
	for i := range gts {
		out[i] = &gurvy381.Gt{GT: gts[i]}
	}
	return out
}

// MulBatchG1 returns a[i].Mul(b[i]) for every i with one kernel launch (the batched form of G1.Mul,
// bls12-381.go:238-247; SURVEY.md 8f row 3).
func (c *Curve) MulBatchG1(a []driver.G1, b []driver.Zr) []driver.G1 {
	n := len(a)
	if len(b) != n {
		panic("hip: MulBatchG1 length mismatch")
	}
	if n == 0 {
		return nil
	}
	points := make([]bls12381.G1Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G1).G1Affine
	}
	return c.scalarMulG1(points, 1, b, false)
}

// MulBatchSubgroupG1 is MulBatchG1 for points the caller knows to be in G1 (decoded with the subgroup check, MSM outputs
// over checked bases, generators and their multiples): the same results from the curve's endomorphism and a split of the
// scalar (mlhip_scalar_mul_subgroup).  A point outside G1 gives an undefined result for its own product; G1.Mul and
// MulBatchG1 accept any point of the curve.  On BN254 every point of the curve is in G1 (the lattice split of DESIGN.md
// section 20 runs): only a point off the curve breaks the promise.
func (c *Curve) MulBatchSubgroupG1(a []driver.G1, b []driver.Zr) []driver.G1 {
	n := len(a)
	if len(b) != n {
		panic("hip: MulBatchSubgroupG1 length mismatch")
	}
	if n == 0 {
		return nil
	}
	points := make([]bls12381.G1Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G1).G1Affine
	}
	return c.scalarMulG1(points, 1, b, true)
}

// BaseMulBatchG1 returns base.Mul(b[i]) for every i: one base (a generator, a Pedersen base), many scalars.  From 2^12
// scalars on the library multiplies through a table of the base's multiples, which it keeps on the device: later calls
// with the same base skip the table's construction.
func (c *Curve) BaseMulBatchG1(base driver.G1, b []driver.Zr) []driver.G1 {
	if len(b) == 0 {
		return nil
	}
	return c.scalarMulG1([]bls12381.G1Affine{base.(*gurvy381.G1).G1Affine}, 0, b, false)
}

func (c *Curve) scalarMulG1(points []bls12381.G1Affine, stride int, b []driver.Zr, subgroup bool) []driver.G1 {
	n := len(b)
	scalars := make([]fr.Element, n)
	for i := range b {
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	res := make([]bls12381.G1Affine, n)
	check(func() C.int {
		if subgroup {
			return C.mlhip_scalar_mul_subgroup(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1,
				unsafe.Pointer(&points[0]), C.size_t(stride), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), unsafe.Pointer(&res[0]))
		}
		return C.mlhip_scalar_mul(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1,
			unsafe.Pointer(&points[0]), C.size_t(stride), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), unsafe.Pointer(&res[0]))
	})
	out := make([]driver.G1, n)
	for i := range res {
		out[i] = &gurvy381.G1{G1Affine: res[i]}
	}
	return out
}

// MulBatchG2 / BaseMulBatchG2: the same for G2 (bls12-381.go:342-351).
func (c *Curve) MulBatchG2(a []driver.G2, b []driver.Zr) []driver.G2 {
	n := len(a)
	if len(b) != n {
		panic("hip: MulBatchG2 length mismatch")
	}
	if n == 0 {
		return nil
	}
	points := make([]bls12381.G2Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G2).G2Affine
	}
	return c.scalarMulG2(points, 1, b, false)
}

// MulBatchSubgroupG2: the same for points the caller knows to be in G2.
func (c *Curve) MulBatchSubgroupG2(a []driver.G2, b []driver.Zr) []driver.G2 {
	n := len(a)
	if len(b) != n {
		panic("hip: MulBatchSubgroupG2 length mismatch")
	}
	if n == 0 {
		return nil
	}
	points := make([]bls12381.G2Affine, n)
	for i := range a {
		points[i] = a[i].(*gurvy381.G2).G2Affine
	}
	return c.scalarMulG2(points, 1, b, true)
}

func (c *Curve) BaseMulBatchG2(base driver.G2, b []driver.Zr) []driver.G2 {
	if len(b) == 0 {
		return nil
	}
	return c.scalarMulG2([]bls12381.G2Affine{base.(*gurvy381.G2).G2Affine}, 0, b, false)
}

func (c *Curve) scalarMulG2(points []bls12381.G2Affine, stride int, b []driver.Zr, subgroup bool) []driver.G2 {
	n := len(b)
	scalars := make([]fr.Element, n)
	for i := range b {
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	res := make([]bls12381.G2Affine, n)
	check(func() C.int {
		if subgroup {
			return C.mlhip_scalar_mul_subgroup(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2,
				unsafe.Pointer(&points[0]), C.size_t(stride), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), unsafe.Pointer(&res[0]))
		}
		return C.mlhip_scalar_mul(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2,
			unsafe.Pointer(&points[0]), C.size_t(stride), unsafe.Pointer(&scalars[0]), 1, C.size_t(n), unsafe.Pointer(&res[0]))
	})
	out := make([]driver.G2, n)
	for i := range res {
		out[i] = &gurvy381.G2{G2Affine: res[i]}
	}
	return out
}

// ExpBatch returns gts[i].Exp(b[i]) for every i with one kernel launch (Gt.Exp, bls12-381.go:399-407; SURVEY.md 8f row 2).
func (c *Curve) ExpBatch(gts []driver.Gt, b []driver.Zr) []driver.Gt {
	n := len(gts)
	if len(b) != n {
		panic("hip: ExpBatch length mismatch")
	}
	if n == 0 {
		return nil
	}
	in := make([]bls12381.GT, n)
	scalars := make([]fr.Element, n)
	for i := range gts {
		in[i] = gts[i].(*gurvy381.Gt).GT
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	res := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_gt_exp(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), unsafe.Pointer(&scalars[0]), 1, C.size_t(n),
			unsafe.Pointer(&res[0]))
	})
	out := make([]driver.Gt, n)
	for i := range res {
		out[i] = &gurvy381.Gt{GT: res[i]}
	}
	return out
}

// ExpBatchGt is ExpBatch for values the caller knows to be members of Gt (FExp outputs, GenGt, products and powers of
// these): the same results from cyclotomic squarings and a Frobenius split of the scalar (mlhip_gt_exp_cyclo).  A value
// outside Gt, such as a Pairing or Pairing2 output before FExp, gives an undefined result; Gt.Exp and ExpBatch accept any.
func (c *Curve) ExpBatchGt(gts []driver.Gt, b []driver.Zr) []driver.Gt {
	n := len(gts)
	if len(b) != n {
		panic("hip: ExpBatchGt length mismatch")
	}
	if n == 0 {
		return nil
	}
	in := make([]bls12381.GT, n)
	scalars := make([]fr.Element, n)
	for i := range gts {
		in[i] = gts[i].(*gurvy381.Gt).GT
		scalars[i] = gurvy381.ZrValue(b[i])
	}
	res := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_gt_exp_cyclo(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), unsafe.Pointer(&scalars[0]), 1, C.size_t(n),
			unsafe.Pointer(&res[0]))
	})
	out := make([]driver.Gt, n)
	for i := range res {
		out[i] = &gurvy381.Gt{GT: res[i]}
	}
	return out
}

// gtStatusError is gnark's message class for a Gt encoding the device refused: 1 = a coordinate >= p, 3 = not in Gt.
func gtStatusError(st byte) string {
	if st == 3 {
		return "set bytes failed [invalid Gt: subgroup check failed]"
	}
	return "set bytes failed [invalid fp.Element encoding]"
}

// NewGtFromBytes decodes gnark's GT.Bytes() on the device (mlhip_gt_from_bytes) without the subgroup check, as GT.SetBytes
// does, and panics like the embedded driver on a malformed encoding (bls12-381.go:571-579).
func (c *Curve) NewGtFromBytes(b []byte) driver.Gt {
	gts, st := c.NewGtFromBytesBatch(b, false)
	if len(gts) != 1 {
		panic("set bytes failed [invalid length]")
	}
	if st[0] != 0 {
		panic(gtStatusError(st[0]))
	}
	return gts[0]
}

// NewGtFromBytesBatch decodes len(raw) / 576 encodings in one call.  With subgroupCheck each value is also tested for
// membership of Gt (mlhip_gt_is_member's test).  statuses[i] is 0 (ok), 1 (malformed) or 3 (not in Gt); a value whose
// status is not 0 is zero.
func (c *Curve) NewGtFromBytesBatch(raw []byte, subgroupCheck bool) ([]driver.Gt, []byte) {
	const sz = bls12381.SizeOfGT
	if len(raw)%sz != 0 {
		panic("set bytes failed [invalid length]")
	}
	n := len(raw) / sz
	if n == 0 {
		return nil, nil
	}
	res := make([]bls12381.GT, n)
	st := make([]byte, n)
	chk := 0
	if subgroupCheck {
		chk = 1
	}
	check(func() C.int {
		return C.mlhip_gt_from_bytes(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&raw[0]), C.size_t(n), C.int(chk),
			unsafe.Pointer(&res[0]), (*C.uchar)(unsafe.Pointer(&st[0])))
	})
	out := make([]driver.Gt, n)
	for i := range res {
		out[i] = &gurvy381.Gt{GT: res[i]}
	}
	return out, st
}

// gtValues copies the values behind a slice of driver.Gt
func gtValues(gts []driver.Gt) []bls12381.GT {
	in := make([]bls12381.GT, len(gts))
	for i := range gts {
		in[i] = gts[i].(*gurvy381.Gt).GT
	}
	return in
}

// GtBytesBatch is Gt.Bytes of every value in one call (mlhip_gt_to_bytes): n x 576 bytes.
func (c *Curve) GtBytesBatch(gts []driver.Gt) []byte {
	n := len(gts)
	if n == 0 {
		return nil
	}
	in := gtValues(gts)
	out := make([]byte, n*bls12381.SizeOfGT)
	check(func() C.int {
		return C.mlhip_gt_to_bytes(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), C.size_t(n), unsafe.Pointer(&out[0]))
	})
	return out
}

// IsInSubGroupBatch reports for every value whether it is a member of Gt (gnark's GT.IsInSubGroup; mlhip_gt_is_member):
// what ExpBatchGt asks its caller to know about a value that arrived as bytes or from another party.
func (c *Curve) IsInSubGroupBatch(gts []driver.Gt) []bool {
	n := len(gts)
	if n == 0 {
		return nil
	}
	in := gtValues(gts)
	st := make([]byte, n)
	check(func() C.int {
		return C.mlhip_gt_is_member(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), C.size_t(n), (*C.uchar)(unsafe.Pointer(&st[0])))
	})
	out := make([]bool, n)
	for i := range st {
		out[i] = st[i] == 0
	}
	return out
}

// InverseBatch is Gt.Inverse of every value in one call, not in place (mlhip_gt_inverse; bls12-381.go:413-415).  Any Fp12
// value is accepted, as by gnark's E12.Inverse; the inverse of 0 is 0.
func (c *Curve) InverseBatch(gts []driver.Gt) []driver.Gt {
	n := len(gts)
	if n == 0 {
		return nil
	}
	in := gtValues(gts)
	res := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_gt_inverse(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&in[0]), C.size_t(n), unsafe.Pointer(&res[0]))
	})
	out := make([]driver.Gt, n)
	for i := range res {
		out[i] = &gurvy381.Gt{GT: res[i]}
	}
	return out
}

// Inverse replaces g by its inverse on the device: Gt.Inverse (bls12-381.go:413-415) for a value of this curve.
func (c *Curve) Inverse(g driver.Gt) {
	v := g.(*gurvy381.Gt)
	check(func() C.int {
		res := v.GT
		rc := C.mlhip_gt_inverse(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&v.GT), 1, unsafe.Pointer(&res))
		v.GT = res
		return rc
	})
}

// NewG1sFromCompressed decodes n compressed G1 points (the wire form of G1.Compressed, bls12-381.go:292-296)
// on the device: decompression, curve check and subgroup check per point.  It is the bulk form of
// NewG1FromCompressed (bls12-381.go:551-559) and panics like it on the first invalid encoding, with gnark's
// message class ("set bytes failed [...]"); the façade's deserializers recover the panic into an error
// (math.go:761-832).
func (c *Curve) NewG1sFromCompressed(raw []byte) []driver.G1 {
	const sz = bls12381.SizeOfG1AffineCompressed
	if len(raw)%sz != 0 {
		panic("set bytes failed [invalid length]")
	}
	n := len(raw) / sz
	if n == 0 {
		return nil
	}
	pts := make([]bls12381.G1Affine, n)
	status := make([]byte, n)
	check(func() C.int {
		return C.mlhip_g1_from_bytes(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&raw[0]), C.size_t(n), 1, 1,
		unsafe.Pointer(&pts[0]), (*C.uchar)(unsafe.Pointer(&status[0])))
	})
	out := make([]driver.G1, n)
	for i := range pts {
		switch status[i] {
		case 0:
			out[i] = &gurvy381.G1{G1Affine: pts[i]}
		case 1:
			panic("set bytes failed [invalid point encoding]")
		case 2:
			panic("set bytes failed [invalid point: not on the curve]")
		default:
			panic("set bytes failed [invalid point: subgroup check failed]")
		}
	}
	return out
}

// G1sCompressed is the inverse: the compressed wire form of every point, concatenated.
func (c *Curve) G1sCompressed(pts []driver.G1) []byte {
	n := len(pts)
	if n == 0 {
		return nil
	}
	aff := make([]bls12381.G1Affine, n)
	for i := range pts {
		aff[i] = pts[i].(*gurvy381.G1).G1Affine
	}
	out := make([]byte, n*bls12381.SizeOfG1AffineCompressed)
	check(func() C.int {
		return C.mlhip_g1_to_bytes(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&aff[0]), C.size_t(n), 1, unsafe.Pointer(&out[0]))
	})
	return out
}

// Bases is a G1 point table kept on the device (SURVEY.md 8f row 1): NewBases uploads it once, MultiScalarMul then
// moves only the scalars (32 bytes each) per call -- the shape of a prover with a fixed SRS.
type Bases struct {
	h *C.mlhip_bases
	n int
}

func (c *Curve) NewBases(points []driver.G1) *Bases {
	n := len(points)
	if n == 0 {
		panic("hip: NewBases needs at least one point")
	}
	aff := make([]bls12381.G1Affine, n)
	for i := range points {
		aff[i] = points[i].(*gurvy381.G1).G1Affine
	}
	b := &Bases{n: n}
	check(func() C.int {
		return C.mlhip_bases_create(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G1, unsafe.Pointer(&aff[0]), C.size_t(n),
		C.int(WindowC), &b.h)
	})
	return b
}

// MultiScalarMul returns sum_i [scalars[i]] bases[i] over the first len(scalars) bases.
func (b *Bases) MultiScalarMul(scalars []driver.Zr) driver.G1 {
	out := &gurvy381.G1{}
	if len(scalars) == 0 {
		return out
	}
	if len(scalars) > b.n {
		panic("hip: more scalars than resident bases")
	}
	sc := make([]fr.Element, len(scalars))
	for i := range scalars {
		sc[i] = gurvy381.ZrValue(scalars[i])
	}
	check(func() C.int {
		return C.mlhip_bases_msm(b.h, unsafe.Pointer(&sc[0]), 1, C.size_t(len(sc)), unsafe.Pointer(&out.G1Affine))
	})
	return out
}

// MultiScalarMulBatch returns, for every i, sum_j [scalars[i][j]] bases[index[i][j]] -- or bases[j] when index is nil, as
// MultiScalarMul does -- in one device call (mlhip_bases_msm_batch: per-base fixed-window tables built on the first call
// that needs them, DESIGN.md section 9).  An idemix / BBS verifier checking many proofs against one issuer key keeps the
// key's bases in one handle.  Without index lists a segment of more scalars than bases panics, as MultiScalarMul does; with
// them every list has as many entries as its scalars and every entry is below the number of bases.
func (b *Bases) MultiScalarMulBatch(scalars [][]driver.Zr, index [][]uint32) []driver.G1 {
	k := len(scalars)
	out := make([]driver.G1, k)
	if k == 0 {
		return out
	}
	if index != nil && len(index) != k {
		panic("hip: MultiScalarMulBatch: as many index lists as scalar lists")
	}
	offsets := make([]uint64, k+1)
	sc := make([]fr.Element, 0, k)
	var idx []uint32
	for i := range scalars {
		if index == nil && len(scalars[i]) > b.n {
			panic("hip: more scalars than resident bases")
		}
		if index != nil {
			if len(index[i]) != len(scalars[i]) {
				panic("hip: MultiScalarMulBatch: as many indices as scalars")
			}
			for _, x := range index[i] {
				if int(x) >= b.n {
					panic("hip: MultiScalarMulBatch: base index out of range")
				}
			}
			idx = append(idx, index[i]...)
		}
		for j := range scalars[i] {
			sc = append(sc, gurvy381.ZrValue(scalars[i][j]))
		}
		offsets[i+1] = offsets[i] + uint64(len(scalars[i]))
	}
	res := make([]bls12381.G1Affine, k)
	var scp unsafe.Pointer
	if len(sc) > 0 {
		scp = unsafe.Pointer(&sc[0])
	}
	var idxp *C.uint32_t
	if len(idx) > 0 {
		idxp = (*C.uint32_t)(unsafe.Pointer(&idx[0]))
	}
	check(func() C.int {
		return C.mlhip_bases_msm_batch(b.h, scp, 1, idxp, (*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.size_t(k),
			unsafe.Pointer(&res[0]))
	})
	for i := range res {
		out[i] = &gurvy381.G1{G1Affine: res[i]}
	}
	return out
}

// SumBatch returns, for every i, sum_j bases[index[i][j]] in one device call (mlhip_bases_sum_batch); with index nil,
// the sum of the first lengths[i] bases.  Every index is below the number of bases and every length at most it; the handle's
// batch tables are neither built nor read.
func (b *Bases) SumBatch(index [][]uint32, lengths []int) []driver.G1 {
	k := len(index)
	if index == nil {
		k = len(lengths)
	}
	out := make([]driver.G1, k)
	if k == 0 {
		return out
	}
	offsets := make([]uint64, k+1)
	var idx []uint32
	for i := 0; i < k; i++ {
		m := 0
		if index != nil {
			for _, x := range index[i] {
				if int(x) >= b.n {
					panic("hip: SumBatch: base index out of range")
				}
			}
			idx = append(idx, index[i]...)
			m = len(index[i])
		} else {
			m = lengths[i]
			if m < 0 || m > b.n {
				panic("hip: SumBatch: more points than resident bases")
			}
		}
		offsets[i+1] = offsets[i] + uint64(m)
	}
	var idxp *C.uint32_t
	if index != nil {
		if len(idx) == 0 {
			idx = []uint32{0}
		}
		idxp = (*C.uint32_t)(unsafe.Pointer(&idx[0]))
	}
	res := make([]bls12381.G1Affine, k)
	check(func() C.int {
		return C.mlhip_bases_sum_batch(b.h, idxp, (*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.size_t(k), unsafe.Pointer(&res[0]))
	})
	for i := range res {
		out[i] = &gurvy381.G1{G1Affine: res[i]}
	}
	return out
}

// CheckedSubgroup reports whether the library verified, on the device, that every point of the table lies in G1.  A
// BLS12-377 table that passes has its bucket sums done in twisted Edwards coordinates (7 field products per addition
// instead of 10); one that does not keeps the Weierstrass kernels and gnark's result for that input.
func (b *Bases) CheckedSubgroup() bool {
	return b.h != nil && C.mlhip_bases_checked_subgroup(b.h) == 1
}

// ShiftedTables reports whether the handle keeps shifted-base tables (include/mlhip.h: mlhip_bases_create): 2^off(j) P_i for
// every digit position, so that all digits of all scalars share one bucket set.
func (b *Bases) ShiftedTables() bool {
	if b.h == nil {
		return false
	}
	p := C.mlhip_bases_plan(b.h)
	if p == nil {
		return false
	}
	var t [11]C.float
	return C.mlhip_msm_plan_timings(p, &t[0], 11) >= 11 && t[10] == 1
}

func (b *Bases) Close() {
	if b.h != nil {
		C.mlhip_bases_destroy(b.h)
		b.h = nil
	}
}

// BasesG2 is a G2 point table kept on the device: Bases for the other group (a Groth16 prover's B2 query).
type BasesG2 struct {
	h *C.mlhip_bases
	n int
}

func (c *Curve) NewBasesG2(points []driver.G2) *BasesG2 {
	n := len(points)
	if n == 0 {
		panic("hip: NewBasesG2 needs at least one point")
	}
	aff := make([]bls12381.G2Affine, n)
	for i := range points {
		aff[i] = points[i].(*gurvy381.G2).G2Affine
	}
	b := &BasesG2{n: n}
	check(func() C.int {
		return C.mlhip_bases_create(C.MLHIP_CURVE_BLS12_381, C.MLHIP_GROUP_G2, unsafe.Pointer(&aff[0]), C.size_t(n),
			C.int(WindowC), &b.h)
	})
	return b
}

func (b *BasesG2) Close() {
	if b.h != nil {
		C.mlhip_bases_destroy(b.h)
		b.h = nil
	}
}

// BasesSet is a set of 1..4 resident tables, G1 and G2 in any order, whose MSMs run over ONE scalar vector from one upload
// and one sort per tile (mlhip_bases_set_create): a Groth16 prover's A, B1 and B2 queries over the witness.  The members
// are not owned: they must stay open while the set is, and stay usable on their own.
type BasesSet struct {
	h      *C.mlhip_bases
	n      int
	groups []int // 1 = G1, 2 = G2, in member order
}

// NewBasesSet takes *Bases and *BasesG2 members.
func (c *Curve) NewBasesSet(members ...interface{}) *BasesSet {
	s := &BasesSet{}
	hs := make([]*C.mlhip_bases, 0, len(members))
	for _, m := range members {
		var h *C.mlhip_bases
		var n, g int
		switch b := m.(type) {
		case *Bases:
			h, n, g = b.h, b.n, 1
		case *BasesG2:
			h, n, g = b.h, b.n, 2
		default:
			panic("hip: NewBasesSet takes *Bases and *BasesG2")
		}
		if len(hs) == 0 || n < s.n {
			s.n = n
		}
		hs = append(hs, h)
		s.groups = append(s.groups, g)
	}
	if len(hs) == 0 {
		panic("hip: NewBasesSet needs at least one member")
	}
	check(func() C.int {
		return C.mlhip_bases_set_create((**C.mlhip_bases)(unsafe.Pointer(&hs[0])), C.size_t(len(hs)), &s.h)
	})
	return s
}

// MultiScalarMul returns every member's MSM over the first len(scalars) bases: the G1 members' results and the G2 members'
// results, each in member order.
func (s *BasesSet) MultiScalarMul(scalars []driver.Zr) ([]driver.G1, []driver.G2) {
	if len(scalars) > s.n {
		panic("hip: more scalars than the smallest member's resident bases")
	}
	const g1b, g2b = 96, 192
	total := 0
	for _, g := range s.groups {
		total += g * g1b
	}
	// (uint64 backing: the results are arrays of 64-bit limbs)
	buf := make([]uint64, total/8)
	sc := make([]fr.Element, len(scalars)+1)
	for i := range scalars {
		sc[i] = gurvy381.ZrValue(scalars[i])
	}
	check(func() C.int {
		return C.mlhip_bases_msm(s.h, unsafe.Pointer(&sc[0]), 1, C.size_t(len(scalars)), unsafe.Pointer(&buf[0]))
	})
	var o1 []driver.G1
	var o2 []driver.G2
	at := 0
	for _, g := range s.groups {
		p := unsafe.Pointer(&buf[at/8])
		if g == 1 {
			o1 = append(o1, &gurvy381.G1{G1Affine: *(*bls12381.G1Affine)(p)})
			at += g1b
		} else {
			o2 = append(o2, &gurvy381.G2{G2Affine: *(*bls12381.G2Affine)(p)})
			at += g2b
		}
	}
	return o1, o2
}

// Route reports how the set's last MultiScalarMul ran: members, sort trains per tile, uploads of the scalar vector, and 1
// when every member read shifted-base tables (mlhip_bases_set_route).
func (s *BasesSet) Route() [4]int {
	var info [4]C.int
	var out [4]int
	if s.h == nil {
		return out
	}
	k := int(C.mlhip_bases_set_route(s.h, &info[0], 4))
	for i := 0; i < k && i < 4; i++ {
		out[i] = int(info[i])
	}
	return out
}

func (s *BasesSet) Close() {
	if s.h != nil {
		C.mlhip_bases_destroy(s.h)
		s.h = nil
	}
}

// G2Prepared holds fixed G2 points with their Miller-loop lines resident on the device (mlhip_g2_prepared_*): the G2
// arguments of the verifier's Pairing2 + FExp (bls12-381.go:448-468), prepared once.
type G2Prepared struct {
	h *C.mlhip_g2_prepared
	m int
}

func (c *Curve) NewG2Prepared(points []driver.G2) *G2Prepared {
	m := len(points)
	if m == 0 {
		panic("hip: NewG2Prepared needs at least one point")
	}
	aff := make([]bls12381.G2Affine, m)
	for i := range points {
		aff[i] = points[i].(*gurvy381.G2).G2Affine
	}
	p := &G2Prepared{m: m}
	check(func() C.int {
		return C.mlhip_g2_prepared_create(C.MLHIP_CURVE_BLS12_381, unsafe.Pointer(&aff[0]), C.size_t(m), &p.h)
	})
	return p
}

// Pairing2Batch returns out[k] = FExp(Pairing2(Q[0], Q[1], p1a[k], p1b[k])) for the handle's first two points: the
// verifier's pairing check over K proofs in one launch (mlhip_pairing_prepared).
func (p *G2Prepared) Pairing2Batch(p1a, p1b []driver.G1) []driver.Gt {
	n := len(p1a)
	if len(p1b) != n {
		panic("hip: Pairing2Batch length mismatch")
	}
	if p.m < 2 {
		panic("hip: Pairing2Batch needs a handle of two points")
	}
	if n == 0 {
		return nil
	}
	g1 := make([]bls12381.G1Affine, 2*n)
	for i := 0; i < n; i++ {
		g1[2*i] = p1a[i].(*gurvy381.G1).G1Affine
		g1[2*i+1] = p1b[i].(*gurvy381.G1).G1Affine
	}
	gts := make([]bls12381.GT, n)
	check(func() C.int {
		return C.mlhip_pairing_prepared(p.h, unsafe.Pointer(&g1[0]), nil, 2, C.size_t(n), unsafe.Pointer(&gts[0]))
	})
	out := make([]driver.Gt, n)
	for i := range gts {
		out[i] = &gurvy381.Gt{GT: gts[i]}
	}
	return out
}

// MillerLoopBatch returns out[k] = prod_j MillerLoop(g1s[k][j], Q[index[j]]) (index nil: Q[j]) for any number of pairs per
// product (mlhip_miller_loop_prepared_products); compare after FExp, as Pairing.
func (p *G2Prepared) MillerLoopBatch(g1s [][]driver.G1, index []uint32) []driver.Gt {
	return p.products(false, g1s, index)
}

// PairingBatch returns out[k] = FExp of the same product (mlhip_pairing_prepared_products).
func (p *G2Prepared) PairingBatch(g1s [][]driver.G1, index []uint32) []driver.Gt {
	return p.products(true, g1s, index)
}

func (p *G2Prepared) products(fused bool, g1s [][]driver.G1, index []uint32) []driver.Gt {
	n := len(g1s)
	if n == 0 {
		return nil
	}
	m := len(g1s[0])
	if m == 0 || (index != nil && len(index) != m) || (index == nil && m > p.m) {
		panic("hip: G2Prepared: one prepared point per pair of a product")
	}
	for _, x := range index {
		if int(x) >= p.m {
			panic("hip: G2Prepared: point index out of range")
		}
	}
	g1 := make([]bls12381.G1Affine, 0, n*m)
	for k := range g1s {
		if len(g1s[k]) != m {
			panic("hip: G2Prepared: every product takes the same number of G1 points")
		}
		for j := 0; j < m; j++ {
			g1 = append(g1, g1s[k][j].(*gurvy381.G1).G1Affine)
		}
	}
	var ix *C.uint32_t
	if index != nil {
		ix = (*C.uint32_t)(unsafe.Pointer(&index[0]))
	}
	gts := make([]bls12381.GT, n)
	check(func() C.int {
		if fused {
			return C.mlhip_pairing_prepared_products(p.h, unsafe.Pointer(&g1[0]), ix, C.size_t(m), C.size_t(n), unsafe.Pointer(&gts[0]))
		}
		return C.mlhip_miller_loop_prepared_products(p.h, unsafe.Pointer(&g1[0]), ix, C.size_t(m), C.size_t(n), unsafe.Pointer(&gts[0]))
	})
	out := make([]driver.Gt, n)
	for i := range gts {
		out[i] = &gurvy381.Gt{GT: gts[i]}
	}
	return out
}

func (p *G2Prepared) Close() {
	if p.h != nil {
		C.mlhip_g2_prepared_destroy(p.h)
		p.h = nil
	}
}
